// mgc_bases.hpp -- ASCII bases -> 2-bit codes + invalid-base masks, four and sixteen at a time.  The kernels of mgc_kmer.hip
// include it (through mgc_common.hpp's types), and so can a plain host program: tests/host/decode_host.cpp compares these forms
// with the expressions they replaced.  No dependency but <cstdint>.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MGC_BASES_FN __host__ __device__ __forceinline__
#else
#define MGC_BASES_FN inline
#endif

namespace mgc {

// 4 ASCII bytes (byte 0 = first base) -> the 2-bit code of every byte, in place: code = (ascii >> 1) & 3 gives A0 C1 T2 G3 for
// both cases
MGC_BASES_FN uint32_t code_bytes4(uint32_t w) { return (w >> 1) & 0x03030303u; }

// ... -> 8 bits of 2-bit codes, first base most significant
MGC_BASES_FN uint32_t enc4_codes(uint32_t cb) { return (cb * 0x40100401u) >> 24; }
MGC_BASES_FN uint32_t enc4(uint32_t w) { return enc4_codes(code_bytes4(w)); }

// byte i of the result = byte sel_i of `table`, sel_i = byte i of `sel` (0..3): one v_perm_b32 on the device
MGC_BASES_FN uint32_t select_bytes4(uint32_t table, uint32_t sel) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_perm(table, table, sel);   // (selectors 0..3 name the bytes of the second source, 4..7 of the first)
#else
  uint32_t r = 0;
  for (int i = 0; i < 4; i++) r |= ((table >> (8u * ((sel >> (8 * i)) & 3u))) & 0xFFu) << (8 * i);
  return r;
#endif
}

// 4 ASCII bytes -> 4-bit mask, bit 3 = byte 0 is NOT one of ACGTacgt.  The code of a byte already names the only letter the byte
// can be ("GTCA"[code], as a byte table 0x47544341): a byte is a base exactly when it equals that letter with the case bit
// folded away -- one select, one xor and one non-zero-byte test instead of a zero-byte test against each of the four letters.
MGC_BASES_FN uint32_t inv4_codes(uint32_t w, uint32_t cb) {
  const uint32_t x  = (w & 0xDFDFDFDFu) ^ select_bytes4(0x47544341u, cb);        // zero bytes: bases
  const uint32_t nz = (((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x) & 0x80808080u;     // 0x80 in every non-zero byte (exact)
  return (((nz >> 7) * 0x08040201u) >> 24) & 0xFu;
}
MGC_BASES_FN uint32_t inv4(uint32_t w) { return inv4_codes(w, code_bytes4(w)); }

// 16 ASCII bytes as four words (x first) -> `codes`: 32 bits of 2-bit codes, first base most significant; `inval`: 16 bits, bit
// 15 = the first byte is no base
MGC_BASES_FN void encode16(uint32_t x, uint32_t y, uint32_t z, uint32_t w, uint32_t &codes, uint32_t &inval) {
  const uint32_t cx = code_bytes4(x), cy = code_bytes4(y), cz = code_bytes4(z), cw = code_bytes4(w);
  codes = (enc4_codes(cx) << 24) | (enc4_codes(cy) << 16) | (enc4_codes(cz) << 8) | enc4_codes(cw);
  inval = (inv4_codes(x, cx) << 12) | (inv4_codes(y, cy) << 8) | (inv4_codes(z, cz) << 4) | inv4_codes(w, cw);
}

}  // namespace mgc
