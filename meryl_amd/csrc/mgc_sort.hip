// mgc_sort.hip -- radix sort / grouping passes (gfx950).
//
// What each kernel replaces in the reference (paths relative to the reference root):
//   kmer_hist_kernel / kmer_partition_kernel
//       kmerIterator + insertKmers            src/meryl/merylOp-countThreads.C:235-280
//       (2-bit pack A0 C1 T2 G3, reverse complement, canonical pick, prefix split;
//        the per-bucket spin-lock + bit-packed append of merylCountArray.C:490-728
//        becomes a histogram + lock-free scatter into per-file regions)
//   radix_* kernels
//       unpack + std::sort of each bucket      src/meryl/merylCountArray.C:276-289,330
//   rle_* kernels
//       the two run-length passes              src/meryl/merylCountArray.C:334-358
//   block_offsets_kernel
//       the per-prefix (prefix, nKmers) split that feeds addBlock
//                                              src/meryl/merylCountArray.C:472-475
//
// All of it is integer / byte work bounded by HBM bandwidth: loads are 16 B (bases) or
// 8 B per lane coalesced, every reorder is staged through LDS so stores leave as
// contiguous runs, ranking uses 64-lane ballots, cross-workgroup prefixes use 8-byte
// {flag,epoch,value} granules with agent-scope relaxed atomics (no fences needed:
// the datum is the flag).  Wave = 64 everywhere.
#include "mgc_common.hpp"
#include "mgc_group_route.hpp"

#include <algorithm>
#include <type_traits>

namespace mgc {

// ============================================================================
//  LSB radix sort of uint64 keys
// ============================================================================
//
// One pass = one stable counting sort on a digit of <= RB bits:
//   * keys of a tile (BLOCK*KPT consecutive keys) are loaded wave-striped, so a
//     wave reads 512 contiguous bytes per instruction;
//   * each wave ranks its keys with RB ballots per key (peers holding the same
//     digit) against a wave-private LDS digit counter -- data-independent cost,
//     stable by construction;
//   * digit totals of the tile are prefix-summed; in ONESWEEP mode the tile's
//     global digit bases come from a decoupled look-back over earlier tiles'
//     8-byte status granules, in CLASSIC mode from a precomputed table;
//   * keys are permuted through LDS into digit order and leave as contiguous
//     runs (one run per digit), i.e. coalesced 8 B/lane stores.
// Algorithmic HBM traffic per pass: 8 B read + 8 B write per key (ONESWEEP; the
// digit histograms of all passes are taken in one extra 8 B/key read up front).

constexpr int      RS_MAX_PASSES = 16;
constexpr int      RS_MAX_RADIX  = 512;
constexpr u32      RS_SPIN_LIMIT = 1u << 24;

struct SortHeader {                       // lives at the start of the sort workspace
  u64 ghist[RS_MAX_PASSES][RS_MAX_RADIX]; // digit counts per pass
  u64 gbase[RS_MAX_PASSES][RS_MAX_RADIX]; // exclusive digit bases per pass
  u32 ticket[RS_MAX_PASSES];
  u32 pad[16];
};

struct PassList { u32 n; u32 shift[RS_MAX_PASSES]; u32 mask[RS_MAX_PASSES]; };

// Digit histograms of every pass in one read of the keys.  NP > 0: exactly NP passes (shifts and masks stay in
// registers, the LDS histogram is NP rows: 4 KiB for the two passes of the finish path, so eight 256-thread
// workgroups fit a CU); NP == 0: any number of passes up to RS_MAX_PASSES.
template <typename K, int NP>
__global__ __launch_bounds__(256)
void radix_hist_kernel(const K *__restrict__ in, u64 n, PassList pl, u64 *__restrict__ ghist) {
  constexpr u32 ROWS = NP ? NP : RS_MAX_PASSES;
  __shared__ u32 s_h[ROWS * RS_MAX_RADIX];
  const u32 np = NP ? (u32)NP : pl.n;
  for (u32 i = threadIdx.x; i < np * RS_MAX_RADIX; i += 256) s_h[i] = 0;
  __syncthreads();

  // 4 independent loads in flight per thread (the loop is otherwise latency-bound)
  constexpr u32 UNR = 4;
  const u64 gstride = (u64)gridDim.x * 256 * UNR;
  for (u64 base = (u64)blockIdx.x * 256 * UNR; base < n; base += gstride) {
    K key[UNR];
    bool ok[UNR];
#pragma unroll
    for (u32 j = 0; j < UNR; j++) {
      const u64 i = base + (u64)j * 256 + threadIdx.x;
      ok[j] = i < n;
      if (ok[j]) key[j] = in[i];
    }
#pragma unroll
    for (u32 j = 0; j < UNR; j++) {
      if (!ok[j]) continue;
      if (NP) {
#pragma unroll
        for (u32 p = 0; p < ROWS; p++)
          atomicAdd(&s_h[p * RS_MAX_RADIX + KeyOps<K>::digit(key[j], pl.shift[p], pl.mask[p])], 1u);
      } else {
        for (u32 p = 0; p < np; p++)
          atomicAdd(&s_h[p * RS_MAX_RADIX + KeyOps<K>::digit(key[j], pl.shift[p], pl.mask[p])], 1u);
      }
    }
  }
  __syncthreads();
  for (u32 i = threadIdx.x; i < np * RS_MAX_RADIX; i += 256) {
    const u32 v = s_h[i];
    if (v) atomicAdd(&ghist[i], (u64)v);
  }
}

template <typename K>
static void launch_radix_hist(const K *src, u64 n, const PassList &pl, u64 *ghist, hipStream_t st) {
  uint64_t hgrid = (n + 256 * 16 - 1) / (256 * 16);
  if (hgrid > 2048) hgrid = 2048;
  const dim3 g((uint32_t)hgrid), b(256);
  switch (pl.n) {
    case 1:  hipLaunchKernelGGL((radix_hist_kernel<K, 1>), g, b, 0, st, src, n, pl, ghist); break;
    case 2:  hipLaunchKernelGGL((radix_hist_kernel<K, 2>), g, b, 0, st, src, n, pl, ghist); break;
    case 3:  hipLaunchKernelGGL((radix_hist_kernel<K, 3>), g, b, 0, st, src, n, pl, ghist); break;
    case 4:  hipLaunchKernelGGL((radix_hist_kernel<K, 4>), g, b, 0, st, src, n, pl, ghist); break;
    default: hipLaunchKernelGGL((radix_hist_kernel<K, 0>), g, b, 0, st, src, n, pl, ghist); break;
  }
}

// Exclusive scan over the digits of each pass (one workgroup per pass).
__global__ __launch_bounds__(RS_MAX_RADIX)
void radix_digit_scan_kernel(const u64 *__restrict__ ghist, u64 *__restrict__ gbase) {
  __shared__ u64 s_tmp[RS_MAX_RADIX / 64 + 1];
  const u32 p = blockIdx.x;
  const u64 v = ghist[(u64)p * RS_MAX_RADIX + threadIdx.x];
  u64 total;
  const u64 e = block_excl_scan<RS_MAX_RADIX, u64>(v, s_tmp, &total);
  gbase[(u64)p * RS_MAX_RADIX + threadIdx.x] = e;
}

__device__ __forceinline__ void status_store(u64 *p, u64 v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ u64 status_load(u64 *p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Look-back status granule: one 8-byte word carries TWO digits, each as
// flag(2) | value(30); flag 1 = tile aggregate, 2 = inclusive prefix.  Half as many
// fabric transactions as one granule per digit, and a digit pair is published by one
// store, so no fence is needed (the datum is the flag).  Values < 2^30: the look-back
// path handles n < 2^30 keys per sort call, larger calls take the classic path.
__device__ __forceinline__ u64 st_pack(u32 f0, u32 v0, u32 f1, u32 v1) {
  return ((u64)((f1 << 30) | v1) << 32) | (u64)((f0 << 30) | v0);
}


template <typename K, int RB, int BLOCK, int KPT, int LB>
struct RadixSmem {
  static constexpr int R     = 1 << RB;
  static constexpr int NW    = BLOCK / 64;
  static constexpr int TILE  = BLOCK * KPT;
  // region 0 is shared between the ranking scratch (wave digit counters u32[NW][R] followed by
  // wave match masks u64[NW][R]) and the key exchange buffer
  static constexpr size_t RANK_BYTES = (size_t)NW * R * 12;
  static constexpr size_t REGION0 = ((size_t)TILE * sizeof(K) > RANK_BYTES) ? (size_t)TILE * sizeof(K) : RANK_BYTES;
  static constexpr size_t OFF_GBASE = REGION0;                     // u64[R]
  static constexpr size_t OFF_DBASE = OFF_GBASE + (size_t)R * 8;   // u32[R]
  static constexpr size_t OFF_CNT   = OFF_DBASE + (size_t)R * 4;   // u32[R]
  static constexpr size_t OFF_TMP   = OFF_CNT + (size_t)R * 4;     // u32[64] scan scratch + misc
  static constexpr size_t OFF_WIN   = OFF_TMP + 64 * 4;            // u64[LB_WINDOW][R/2] look-back window (LB == 2)
  static constexpr size_t WIN_BYTES = 8192;
  static constexpr size_t BYTES     = OFF_WIN + WIN_BYTES;
  // workgroups per CU the LDS budget admits (160 KiB per CU), capped at 2
  static constexpr int    WG_PER_CU = (2 * BYTES <= 160 * 1024) ? 2 : 1;
  static constexpr int    MIN_WAVES_PER_SIMD = (WG_PER_CU * BLOCK) / 256;
};

// LB 2: two digits per look-back granule (30-bit values, n < 2^30); LB 3: one digit per granule (62-bit values)
template <typename K, int RB, int BLOCK, int KPT, int LB>
__global__ __launch_bounds__(BLOCK, (RadixSmem<K, RB, BLOCK, KPT, LB>::MIN_WAVES_PER_SIMD))
void radix_scatter_kernel(const K *__restrict__ in, K *__restrict__ out, u64 n, u32 shift, u32 dmask,
                          const u64 *__restrict__ gbase,      // exclusive digit bases of this pass
                          u64 *__restrict__ status,           // [num_tiles][R/2 or R] granules of this pass (zeroed)
                          u32 *__restrict__ ticket, u32 *__restrict__ error_flag) {
  static_assert(LB == 2 || LB == 3, "window look-back with packed or wide granules");
  using SM = RadixSmem<K, RB, BLOCK, KPT, LB>;
  using KO = KeyOps<K>;
  constexpr int R = SM::R, NW = SM::NW, TILE = SM::TILE;
  static_assert(BLOCK >= R, "one thread per digit needed");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  K   *s_keys  = reinterpret_cast<K *>(smem);
  u32 *s_whist = reinterpret_cast<u32 *>(smem);                       // aliases s_keys (see barriers)
  u64 *s_gbase = reinterpret_cast<u64 *>(smem + SM::OFF_GBASE);
  u32 *s_dbase = reinterpret_cast<u32 *>(smem + SM::OFF_DBASE);
  u32 *s_cnt   = reinterpret_cast<u32 *>(smem + SM::OFF_CNT);
  u32 *s_tmp   = reinterpret_cast<u32 *>(smem + SM::OFF_TMP);

  const u32 tid = threadIdx.x, lane = lane_id(), w = wave_id();

  // Tile ids are tickets: every lower-numbered tile has started, hence is resident and will
  // publish its aggregate -- the look-back cannot deadlock (spins are bounded anyway).
  if (tid == 0) s_tmp[32] = atomicAdd(ticket, 1u);
  __syncthreads();
  const u64 tile = s_tmp[32];

  for (u32 i = tid; i < (u32)(NW * R * 3); i += BLOCK) s_whist[i] = 0;   // counters + match masks
  __syncthreads();

  // ---- load (wave-striped: 512 contiguous bytes per wave instruction) ----
  const u64  tile_base = tile * (u64)TILE;
  const bool full      = (tile_base + TILE <= n);
  const u64  wave_base = tile_base + (u64)w * (64 * KPT) + lane;
  K keys[KPT];
#pragma unroll
  for (int j = 0; j < KPT; j++) {
    const u64 idx = wave_base + (u64)j * 64;
    keys[j] = (full || idx < n) ? in[idx] : KO::pad();  // padding sorts to the end of the last digit
  }

  // ---- rank inside the wave (stable: by lane order inside a row, rows in order) ----
  const u64 lt_mask = (1ull << lane) - 1ull;
  u32 ranks[KPT / 2];                                  // two 16-bit ranks per register (rank < TILE <= 2^14)
  {
    // peers through a wave-private LDS mask per digit: every lane ORs its lane bit into
    // mask[digit], reads the mask back (LDS executes a wave's instructions in order), and the
    // lowest peer bumps the running digit counter and clears the mask for the next row.
    lds_u32 *wh = (lds_u32 *)(smem) + w * R;
    lds_u64 *mk = (lds_u64 *)(smem + (size_t)NW * R * 4) + w * R;
    const u64 lane_bit = 1ull << lane;
#pragma unroll
    for (int j = 0; j < KPT; j++) {
      const u32 d = KO::digit(keys[j], shift, dmask);
      __hip_atomic_fetch_or(&mk[d], lane_bit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
      const u64 peers = __hip_atomic_load(&mk[d], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
      const u32 base  = __hip_atomic_load(&wh[d], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
      const u32 lower = __popcll(peers & lt_mask);
      if (lower == 0) {
        __hip_atomic_store(&wh[d], base + (u32)__popcll(peers), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
        __hip_atomic_store(&mk[d], 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
      }
      if (j & 1) ranks[j / 2] |= (base + lower) << 16;
      else       ranks[j / 2]  = (base + lower);
    }
  }
  __syncthreads();

  // ---- digit totals of the tile, wave-exclusive bases ----
  const u32 n_valid = full ? (u32)TILE : (u32)(n - tile_base);
  u32 count = 0;
  if (tid < (u32)R) {
    u32 acc = 0;
#pragma unroll
    for (int ww = 0; ww < NW; ww++) {
      const u32 t = s_whist[ww * R + tid];
      s_whist[ww * R + tid] = acc;
      acc += t;
    }
    count = acc;
    // padding keys all carry the top digit; they are not published to later tiles
    s_cnt[tid] = (tid == dmask) ? count - ((u32)TILE - n_valid) : count;
  }
  u32 tile_total;
  const u32 excl = block_excl_scan<BLOCK, u32>(count, s_tmp, &tile_total);
  if (tid < (u32)R) s_dbase[tid] = excl;

  // granules of this tile: publish the aggregate as early as possible
  constexpr int GW = (LB == 3) ? 1 : 2;                 // digits per granule
  constexpr int G  = R / GW;                            // granules per tile
  constexpr u64 V62 = (1ull << 62) - 1;
  u64 *mine = status + tile * (u64)G + tid;
  __syncthreads();                                      // s_cnt / s_dbase visible
  if (tid < (u32)G) {
    const u32 c0 = s_cnt[GW * tid], c1 = (GW == 2) ? s_cnt[GW * tid + 1] : 0u;
    const u32 fl = (tile == 0) ? 2u : 1u;
    status_store(mine, (GW == 2) ? st_pack(fl, c0, fl, c1) : (((u64)fl << 62) | (u64)c0));
  }

  // ---- final position of every key inside the sorted tile ----
#pragma unroll
  for (int j = 0; j < KPT; j++) {           // ranks[] becomes positions in place (still < TILE)
    const u32 d = KO::digit(keys[j], shift, dmask);
    const u32 add = s_dbase[d] + s_whist[w * R + d];
    ranks[j / 2] += (j & 1) ? (add << 16) : add;
  }
  __syncthreads();                          // s_whist is dead; its storage becomes s_keys
#pragma unroll
  for (int j = 0; j < KPT; j++) s_keys[(j & 1) ? (ranks[j / 2] >> 16) : (ranks[j / 2] & 0xFFFFu)] = keys[j];
  __syncthreads();                          // keys now live in LDS only: registers are free for the look-back

  {
    // window-parallel look-back after the exchange (keys live in LDS only, registers are free):
    // all waves fetch the granules of the next LB_WINDOW predecessors with coalesced loads into
    // LDS, the R/2 digit-pair threads consume the ready prefix.
    constexpr int TPL = BLOCK / G;                      // predecessor tiles covered by one load per thread
    constexpr int WIN0 = (int)(SM::WIN_BYTES / ((size_t)G * 8));
    constexpr int LB_WINDOW = (WIN0 < TPL) ? TPL : WIN0;
    constexpr int LPT = LB_WINDOW / TPL;
    static_assert(LB_WINDOW % TPL == 0 && LPT >= 1, "window must be a multiple of the tiles one load covers");
    static_assert((size_t)LB_WINDOW * G * 8 <= SM::WIN_BYTES, "look-back window does not fit");
    u64 *s_win = reinterpret_cast<u64 *>(smem + SM::OFF_WIN);
    u32 *s_q   = s_tmp + 40;
    u32 *s_all = s_tmp + 41;
    u32 c0 = 0, c1 = 0;
    u64 p0 = 0, p1 = 0;
    bool need0 = false, need1 = false;
    if (tid < (u32)G) {
      c0 = s_cnt[GW * tid]; c1 = (GW == 2) ? s_cnt[GW * tid + 1] : 0u;
      need0 = (tile != 0);
      need1 = (GW == 2) && (tile != 0);
    }
    if (tile != 0) {                                    // uniform
      const u32 sub = tid / G, g = tid % G;
      u64 t_next = tile - 1;
      u32 spins = 0;
      while (true) {
#pragma unroll
        for (int i = 0; i < LPT; i++) {
          const u32 idx = sub + (u32)(TPL * i);
          s_win[idx * G + g] = (t_next >= (u64)idx) ? status_load(status + (t_next - idx) * (u64)G + g)
                                                    : ((GW == 2) ? st_pack(2, 0, 2, 0) : (2ull << 62));
        }
        if (tid == 0) { *s_q = LB_WINDOW; *s_all = 1u; }
        __syncthreads();
        if (tid < (u32)G) {
          u32 q = 0;
          for (; q < (u32)LB_WINDOW; q++) {
            const u64 v = s_win[q * G + tid];
            if ((GW == 2 && ((u32)v >> 30) == 0u) || ((u32)(v >> 62)) == 0u) break;
          }
          if (q < (u32)LB_WINDOW) atomicMin(s_q, q);
        }
        __syncthreads();
        const u32 q = *s_q;
        if (tid < (u32)G) {
          for (u32 i = 0; i < q && (need0 || need1); i++) {
            const u64 v = s_win[i * G + tid];
            if (GW == 2) {
              const u32 lo = (u32)v, hi = (u32)(v >> 32);
              if (need0) { p0 += lo & 0x3FFFFFFFu; if ((lo >> 30) == 2u) need0 = false; }
              if (need1) { p1 += hi & 0x3FFFFFFFu; if ((hi >> 30) == 2u) need1 = false; }
            } else {
              p0 += v & V62;
              if ((v >> 62) == 2ull) need0 = false;
            }
          }
          if (need0 || need1) *s_all = 0u;
        }
        __syncthreads();
        if (*s_all) break;
        t_next -= (q <= t_next) ? q : t_next;
        if (q == 0) {
          if (++spins > RS_SPIN_LIMIT) { if (tid == 0) atomicExch(error_flag, 1u); break; }
          __builtin_amdgcn_s_sleep(2);
        }
        __syncthreads();
      }
    }
    if (tid < (u32)G) {
      if (tile != 0)
        status_store(mine, (GW == 2) ? st_pack(2, (u32)p0 + c0, 2, (u32)p1 + c1) : ((2ull << 62) | (p0 + (u64)c0)));
      s_gbase[GW * tid] = gbase[GW * tid] + p0 - (u64)s_dbase[GW * tid];
      if (GW == 2) s_gbase[2 * tid + 1] = gbase[2 * tid + 1] + p1 - (u64)s_dbase[2 * tid + 1];
    }
    __syncthreads();
  }

  // ---- contiguous runs leave coalesced ----
#pragma unroll
  for (int j = 0; j < KPT; j++) {
    const u32 i = (u32)j * BLOCK + tid;
    if (i < n_valid) {
      const K   key = s_keys[i];
      const u32 d   = KO::digit(key, shift, dmask);
      out[s_gbase[d] + (u64)i] = key;
    }
  }
}

// ---- grouping pass (plan.mode == 3; the sub-bucket finish path) -----------------------
// The finish path does not need a sorted file, only its k-mers GROUPED by their top bits: sub-bucket
// members may come in any order (the LDS finish counts them anyway).  A grouping pass therefore ranks
// a tile with one returning LDS atomic per key -- no wave-private counters, no match masks, a 2 KiB
// histogram to clear instead of 96 KiB -- and only has to respect the TILE order for the bases.
// With two digits (d_hi:d_lo, LSD): pass 1 groups by d_lo with plain tiles; pass 2 must keep the d_lo
// order inside a d_hi group, which holds if no tile of pass 2 mixes two d_lo values: its tiles are cut
// at the d_lo region boundaries of pass 1's output (region table below), every region's last tile
// being partial.  Persistent workgroups, ticket one tile ahead, next tile's keys fetched behind the
// look-back and the write-out, as in radix_scatter_pipe_kernel.
// XB: bytes per key of the exchange buffer -- sizeof(K) for whole keys; a NARROWING pass exchanges what it writes (group_xb below)
template <typename K, int RB, int BLOCK, int KPT, int XB = (int)sizeof(K)>
struct GroupSmem {
  static constexpr int R = 1 << RB, NW = BLOCK / 64, TILE = BLOCK * KPT;
  static constexpr size_t OFF_HIST  = ((size_t)TILE * XB + 15) / 16 * 16;   // u32[R]
  static constexpr size_t OFF_GBASE = OFF_HIST + (size_t)R * 4;       // u64[R]
  static constexpr size_t OFF_DBASE = OFF_GBASE + (size_t)R * 8;      // u32[R]
  static constexpr size_t OFF_CNT   = OFF_DBASE + (size_t)R * 4;      // u32[R]
  static constexpr size_t OFF_TMP   = OFF_CNT + (size_t)R * 4;        // u32[64]
  static constexpr size_t OFF_INFO  = OFF_TMP + 64 * 4;               // u64[4]: key base / valid count of current+next tile
  static constexpr size_t BYTES     = OFF_INFO + 4 * 8;
  static constexpr int    WG_PER_CU = (2 * BYTES <= 160 * 1024) ? 2 : 1;
  static constexpr int    MIN_WAVES_PER_SIMD = (WG_PER_CU * BLOCK) / 256;
};

// region table of a second grouping pass: regions = digit groups of the first pass (gbase_prev = its
// exclusive digit bases, RS_MAX_RADIX entries, unused digits sit at n)
__global__ __launch_bounds__(RS_MAX_RADIX)
void group_regions_kernel(const u64 *__restrict__ gbase_prev, u64 n, u32 tile, u64 *__restrict__ region_start,
                          u32 *__restrict__ region_tiles) {
  __shared__ u32 s_tmp[RS_MAX_RADIX / 64 + 1];
  const u32 r = threadIdx.x;
  const u64 a = gbase_prev[r], b = (r + 1 < RS_MAX_RADIX) ? gbase_prev[r + 1] : n;
  const u32 nt = (u32)((b - a + tile - 1) / tile);
  u32 total;
  const u32 e = block_excl_scan<RS_MAX_RADIX, u32>(nt, s_tmp, &total);
  region_start[r] = a;
  region_tiles[r] = e;
  if (r == 0) { region_start[RS_MAX_RADIX] = n; region_tiles[RS_MAX_RADIX] = total; }
}

// NARROW (u64 keys only): the keys leave as 32-bit words WITHOUT the digit of this pass -- ((key >> (shift + digit_bits))
// << shift) | low `shift` bits -- because where a key lies now tells its digit (launch_group_narrow): every later pass and
// the finish move half the bytes.
template <typename K, bool NARROW> struct GroupOut { typedef K type; };
template <> struct GroupOut<u64, true> { typedef u32 type; };
// A narrowing pass exchanges what it writes: a key goes through LDS as its 32-bit narrowed word plus its digit of this pass -- u32[TILE]
// words, then the digits, one byte each for digits of up to eight bits (5 bytes per key; the judged plan), 16 bits each for nine-bit
// digits (6 bytes per key) -- instead of the whole 8-byte key, of which 36 bits are live at k = 21.  Every plan that narrows has room
// for that (the word is what leaves the kernel anyway), so no narrowing instantiation keeps the whole-key exchange.
template <typename K, int RB, bool NARROW> constexpr int group_xb() { return NARROW ? (RB <= 8 ? 5 : 6) : (int)sizeof(K); }

// HIST2: the pass also takes the histogram of ANOTHER digit (the next pass's) of the keys it reads -- 512 LDS counters per
// workgroup, flushed with global atomics at the end -- so that nobody has to read the keys for it.
struct GroupExtra { u32 digit_bits /* NARROW */; u32 shift2, mask2; u64 *ghist2 /* HIST2 */;
                    u32 soa_hi_mask = 0 /* SOA: payload bits of the u8 array */;
                    u32 stagger_groups = 0, stagger_cycles = 0 /* STAGGER below: groups, cycles between two groups' starts */; };

// SOA (u64 keys): `in` is the 5-byte layout kmer_partition_kernel<SOA> leaves -- u32 in[n] low words, then u8[n] bits 32..39 --
// and a key is put together as it is fetched: four keys per lane and group from one 16-byte and one 4-byte load.
// PIPE (round 6; the 5-byte first pass): the tile AFTER the next one is fetched -- into registers, in the form it has in memory (5 bytes
// per key: 20 registers for 16 keys) -- a WHOLE tile ahead: its loads are issued behind the write-out of the current tile and are consumed
// behind the look-back of the NEXT one, so they are in flight beside a tile's ranking, scan and exchange as well (round 5's form asks for
// the next tile at the start of the look-back and waits for it at the next ranking: the persistent workgroups, in step because of the
// look-back chain, left the read side of the memory system idle for a third of a tile's time).  Tickets run two tiles ahead.
// Measured (profiles/r06_pipe_ab.txt): first pass 0.545 -> 0.465 ms per launch.  The 32-bit second pass LOSES with the same change
// (0.355 -> 0.385 / 0.45 ms at 20 words per thread: its walkers' wait for the staged words also waits for the granule they have just
// published -- stores count in vmcnt on gfx9 -- and 24 + 24 words per thread do not fit the register file): it keeps round 5's form.
// HPCD (round 6; `compress`): both digits are dense ranks (hpc_digit: ~30 VALU instructions, taken three times per key and pass plus once
// for HIST2 -- the whole-key passes of `compress` were VALU-bound at 0.357 ms per 69 M keys against 0.266 ms for plain bit digits): the
// 4096 ranks of the twelve bits a digit is taken from lie in 8 KiB of LDS behind the tile, a digit is one 16-bit LDS read.
//
// BATCH: ONE launch runs a pass over the tiles of MANY files (the arguments that belong to a file are unused: `n` is the number of files
// and `region_start` points at their descriptors -- the argument list, and with it the code of every per-file instantiation, is the
// one it was: profiles/group_batch_parity.txt).  The launch has one dense ticket sequence over
// the tiles of all its files; a table of per-file descriptors in global memory (GroupBatchFile, bfiles[nbf + 1]) says where a file's
// tiles start in that sequence, and everything that belongs to a file rather than to the launch -- its keys, its output, its digit
// bases, its look-back rows, the other digit's histogram, a second pass's regions -- comes from the descriptor of the file a tile lies
// in.  The shifts and digit widths are the launch's: only files with the same plan digits share a launch.  A workgroup's tickets only
// grow, so the file of an announced tile is found by walking forward from the file of the tile announced before it.  Row numbers of
// the look-back are tile numbers INSIDE the file: a file's first tile publishes its inclusive prefix at once and no walker reads a row
// of another file.  HIST2: the counters are flushed to the file's histogram and cleared when a workgroup's current tile leaves a file.
// PROGRESS (the argument of the per-file launch, unchanged): tickets are dense and only handed to workgroups that run; a tile waits
// only for earlier tiles of its own file; those have smaller tickets, so they are held by running workgroups (or are done), and the
// tile with the smallest ticket that is not done waits for nobody.  The spin is bounded as before (RS_SPIN_LIMIT, the error flag),
// and nothing here spins on what another launch produces: a batch's second pass is a launch of its own behind the first in stream order.
struct GroupBatchFile {
  u64 tile0;                                 // the file's first tile in the launch's ticket sequence; entry [nbf]: the tiles of all files
  u64 tiles;                                 // (second pass: its tile count, from which narrow_mid_batch_kernel makes tile0)
  u64 n;
  const void *in; void *out;
  u64 *gbase, *status, *ghist2;
  u64 *region_start; u32 *region_tiles;      // a second pass's regions (written by narrow_mid_batch_kernel)
  u64 *sub_starts;                           // where narrow_bounds_batch_kernel leaves the sub-bucket boundaries
};

template <typename K, int RB, int BLOCK, int KPT, bool DBG, bool NARROW = false, bool HIST2 = false, bool SOA = false, int PIPE = 0 /* 1: the next fetch before the write-out; 2: after it */,
          int HPCD = 0 /* 1: both digits are dense ranks; 2: only this pass's (the other digit, HIST2's, is a plain bit field) */,
          bool BATCH = false /* the tiles of many files: `n` files, their descriptors in place of region_start, every other per-file argument unused */>
__global__ __launch_bounds__(BLOCK, (GroupSmem<K, RB, BLOCK, KPT, group_xb<K, RB, NARROW>()>::MIN_WAVES_PER_SIMD))
void radix_group_kernel(const K *__restrict__ in, typename GroupOut<K, NARROW>::type *__restrict__ out, u64 n, u32 shift, u32 dmask,
                        const u64 *__restrict__ gbase, u64 *__restrict__ status, u32 *__restrict__ ticket,
                        u32 *__restrict__ error_flag, u64 num_tiles_plain,
                        const u64 *__restrict__ region_start,   // [RS_MAX_RADIX + 1] or nullptr (plain tiles); BATCH: GroupBatchFile[n + 1]
                        const u32 *__restrict__ region_tiles,   // [RS_MAX_RADIX + 1] exclusive; last = total tiles
                        GroupExtra ex, u64 *__restrict__ dbg) {
  // BATCH: the files' descriptors and their number ([nbf] closes the tile sequence)
  const GroupBatchFile *__restrict__ bfiles = BATCH ? reinterpret_cast<const GroupBatchFile *>(region_start) : nullptr;
  const u32 nbf = BATCH ? (u32)n : 0u;
  const u32 digit_bits = ex.digit_bits;
  static_assert(!BATCH || (!DBG && !HPCD), "the batched forms: the judged plan's two passes");
  __shared__ u32 s_h2[HIST2 ? RS_MAX_RADIX : 1];
  if (HIST2) { for (u32 i = threadIdx.x; i < (u32)RS_MAX_RADIX; i += BLOCK) s_h2[i] = 0; }
  using SM = GroupSmem<K, RB, BLOCK, KPT, group_xb<K, RB, NARROW>()>;
  using KO = KeyOps<K>;
  constexpr int R = SM::R, TILE = SM::TILE, G = R / 2;
  static_assert(!NARROW || !HPCD, "dense-rank digits keep whole keys");
  constexpr int WALK = (sizeof(K) == 4 || PIPE) ? 8 : 16;      // 32 words per thread leave registers for eight granules in flight, not sixteen (no spills)
  static_assert(BLOCK >= RS_MAX_RADIX && G % 64 == 0 && TILE <= 65536, "one thread per region/digit; 16-bit ranks");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  K   *s_keys  = reinterpret_cast<K *>(smem);
  // NARROW: the exchange buffer holds the narrowed words and, behind them, the digits of this pass
  using DT = typename std::conditional<(RB <= 8), uint8_t, unsigned short>::type;
  u32 *s_words = reinterpret_cast<u32 *>(smem);
  DT  *s_dig   = reinterpret_cast<DT *>(smem + (NARROW ? (size_t)TILE * 4 : 0));
  u32 *s_hist  = reinterpret_cast<u32 *>(smem + SM::OFF_HIST);
  u64 *s_gbase = reinterpret_cast<u64 *>(smem + SM::OFF_GBASE);
  u32 *s_dbase = reinterpret_cast<u32 *>(smem + SM::OFF_DBASE);
  u32 *s_cnt   = reinterpret_cast<u32 *>(smem + SM::OFF_CNT);
  u32 *s_tmp   = reinterpret_cast<u32 *>(smem + SM::OFF_TMP);
  u64 *s_info  = reinterpret_cast<u64 *>(smem + SM::OFF_INFO);
  const u32 tid0 = threadIdx.x;
  u32 tid = tid0, lane = tid0 & 63u, w = tid0 >> 6;
  static_assert(!HPCD || SM::BYTES + 8192 <= 160 * 1024, "the rank table lies behind the tile");
  unsigned short *s_rank = reinterpret_cast<unsigned short *>(smem + (HPCD ? SM::BYTES : 0));
  if constexpr (HPCD) { for (u32 i = tid0; i < 4096u; i += BLOCK) s_rank[i] = (unsigned short)hpc_digit(i); }   // (in place at the first barrier below)
  auto dig  = [&](const K &key) __attribute__((always_inline)) -> u32 {
    if constexpr (HPCD) return (u32)s_rank[KO::digit(key, shift, 0xFFFu)];
    else return KO::digit(key, shift, dmask);
  };
  auto dig2 = [&](const K &key) __attribute__((always_inline)) -> u32 {
    if constexpr (HPCD == 1) return (u32)s_rank[KO::digit(key, ex.shift2, 0xFFFu)];
    else return KO::digit(key, ex.shift2, ex.mask2);
  };

  // this thread's slice of the region table stays in registers
  // (a narrowing pass is a first pass: plain tiles -- known at compile time, so that the region slice below costs it no registers: the
  // 5-byte pass spilled them and reloaded them at the top of every tile behind an s_waitcnt vmcnt(0), i.e. behind its own prefetch)
  const bool regions = !NARROW && (BATCH || region_tiles != nullptr);
  u64 rt_lo = 0, rt_hi = 0, rs = 0, re = 0, total_tiles = num_tiles_plain;
  // BATCH: the slice is that of file `af`, the file of the tile announced last; it is loaded again when an announced tile lies in
  // another file (the same for all threads: tickets are the workgroup's)
  u32 af = 0;
  auto load_regions = [&](const u64 *rsp, const u32 *rtp) __attribute__((always_inline)) {
    if (tid0 < (u32)RS_MAX_RADIX) {
      rt_lo = rtp[tid0]; rt_hi = rtp[tid0 + 1];
      rs = rsp[tid0];    re = rsp[tid0 + 1];
    }
  };
  if constexpr (BATCH) {
    total_tiles = bfiles[nbf].tile0;
    if (regions) load_regions(bfiles[0].region_start, bfiles[0].region_tiles);
  } else if (regions) {
    if (tid0 < (u32)RS_MAX_RADIX) {
      rt_lo = region_tiles[tid0]; rt_hi = region_tiles[tid0 + 1];
      rs = region_start[tid0];    re = region_start[tid0 + 1];
    }
    total_tiles = region_tiles[RS_MAX_RADIX];
  }
  // (values, not branches over the captured variables: the two-branch form made the compiler select between the ADDRESSES of `re` and
  // `n` -- both in scratch for it, 40 bytes per thread -- and the announcing thread's wave reloaded them behind an s_waitcnt vmcnt(0),
  // i.e. behind its write-out stores, at the top of every tile: round 6, found in the ISA)
  auto announce = [&](u64 t, int slot) __attribute__((always_inline)) {   // key range of tile t -> s_info[2*slot..]
    if (t >= total_tiles) return;
    if constexpr (BATCH) {
      // the tile's file and its number inside the file go along in s_tmp[40 + 2 * slot ..] (the scans use s_tmp[0 .. 16], the tickets
      // s_tmp[32 .. 34]); t < bfiles[nbf].tile0 ends the walk, files without tiles are walked over
      const u32 tu = __builtin_amdgcn_readfirstlane((u32)t);
      u32 f = af;
      while ((u64)tu >= bfiles[f + 1].tile0) f++;
      if (regions && f != af) load_regions(bfiles[f].region_start, bfiles[f].region_tiles);
      af = f;
      const u64 lt = (u64)tu - bfiles[f].tile0;
      const bool mine = regions ? (rt_lo <= lt && lt < rt_hi) : (tid0 == 0);
      const u64  kb   = regions ? rs + (lt - rt_lo) * (u64)TILE : lt * (u64)TILE;
      const u64  endk = regions ? re : bfiles[f].n;
      if (mine) {
        s_info[2 * slot] = kb;
        s_info[2 * slot + 1] = (endk - kb < (u64)TILE) ? endk - kb : (u64)TILE;
        s_tmp[40 + 2 * slot] = f;
        s_tmp[41 + 2 * slot] = (u32)lt;
      }
      return;
    }
    const bool mine = regions ? (rt_lo <= t && t < rt_hi) : (tid0 == 0);   // exactly one thread (empty regions own no tile)
    const u64  kb   = regions ? rs + (t - rt_lo) * (u64)TILE : t * (u64)TILE;
    const u64  endk = regions ? re : n;
    if (mine) {
      s_info[2 * slot] = kb;
      s_info[2 * slot + 1] = (endk - kb < (u64)TILE) ? endk - kb : (u64)TILE;
    }
  };

  // Loads are wave-striped 16-byte vectors (VEC keys per lane and instruction: 1 KiB contiguous per wave instruction).  Fewer,
  // wider loads matter beyond issue slots: the walkers' granule loads queue behind the prefetch of the other twelve waves in
  // the CU's own memory pipeline, by INSTRUCTION -- with 4-byte loads of 32-bit words the look-back took 45 K cycles per tile
  // instead of 17 K (profiles/r02x_groupdbg.log).  Key j of a thread is element idx_of(j) of the tile; order inside a tile is free.
  static_assert(!SOA || (sizeof(K) == 8 && KPT % 4 == 0), "the 5-byte layout holds 8-byte keys");
  // (12-byte K96 records: four per lane and group = three 16-byte loads)
  constexpr int VEC = SOA ? 4 : (sizeof(K) == 12 ? (KPT % 4 == 0 ? 4 : 1) : ((sizeof(K) < 16 && KPT % (16 / sizeof(K)) == 0) ? (int)(16 / sizeof(K)) : 1));
  struct __attribute__((aligned(4))) KVec { K v[VEC]; };     // 4-byte alignment is all a file / region start guarantees
  auto idx_of = [&](int j) __attribute__((always_inline)) -> u32 {
    return w * (u32)(64 * KPT) + ((u32)(j / VEC) * 64u + lane) * (u32)VEC + (u32)(j % VEC);
  };
  K keys[KPT];
  // NARROW: once put together a key lives as word + digit -- narrowed ONCE; ranking, exchange and write-out take the stored digit -- the
  // digits DPR to a register: 24 keys per thread are 24 + 6 registers at eight-bit digits, not 48 (keys[] then only holds what a
  // fetch that is not PIPE's has brought in, until the ranking narrows it)
  constexpr int DPR = (RB <= 8) ? 4 : 2, DBITS = 32 / DPR;
  static_assert(!NARROW || KPT % DPR == 0, "whole registers of digits");
  u32 wd[NARROW ? KPT : 1], dgp[NARROW ? KPT / DPR : 1];
  if constexpr (NARROW) {
#pragma unroll
    for (int j = 0; j < KPT; j++) wd[j] = 0u;
#pragma unroll
    for (int j = 0; j < KPT / DPR; j++) dgp[j] = 0u;
  }
  // (32-bit operations on the key's halves -- one v_alignbit_b32 per field -- instead of 64-bit shifts on register pairs; the shift
  // amounts are the same in all lanes.  sort_plan_narrows: shift <= 32, so the bits below the digit come from the low half alone.)
  auto bits_from = [&](u32 hi, u32 lo, u32 at) __attribute__((always_inline)) -> u32 {      // bits at .. at + 31 of hi:lo
    return at < 32u ? __builtin_amdgcn_alignbit(hi, lo, at) : (at < 64u ? hi >> (at - 32u) : 0u);
  };
  const u32 low_mask = shift < 32u ? (1u << shift) - 1u : 0xFFFFFFFFu;
  auto narrow_to = [&](int j, u32 hi, u32 lo) __attribute__((always_inline)) {
    const u32 up = bits_from(hi, lo, shift + digit_bits);
    wd[j] = (shift < 32u ? up << shift : 0u) | (lo & low_mask);
    const u32 d = bits_from(hi, lo, shift) & dmask;
    if (j % DPR) dgp[j / DPR] |= d << (DBITS * (j % DPR));
    else         dgp[j / DPR]  = d;
  };
  auto dig_of = [&](int j) __attribute__((always_inline)) -> u32 { return (dgp[j / DPR] >> (DBITS * (j % DPR))) & ((1u << DBITS) - 1u); };
  // HIST2 of a narrowing pass counts the other digit from the WORDS: below this pass's digit it sits where it sat in the key
  const u32 shift2w = (ex.shift2 >= shift + digit_bits) ? ex.shift2 - digit_bits : ex.shift2;
  // the file the fetches read: the launch's; BATCH: that of the tile a fetch is issued for (fetch_from)
  const K *in_f = in;
  u64 n_f = n;
  auto fetch_from = [&](u32 f) __attribute__((always_inline)) {
    if constexpr (BATCH) { in_f = reinterpret_cast<const K *>(bfiles[f].in); n_f = bfiles[f].n; }
  };
  auto fetch = [&](u64 kb, u32 nv) __attribute__((always_inline)) {
    if constexpr (SOA) {
      struct __attribute__((aligned(4))) LVec { u32 v[4]; };
      struct __attribute__((packed, aligned(1))) HWord { u32 v; };
      const u32 *lo32 = reinterpret_cast<const u32 *>(in_f) + kb;
      const uint8_t *hi8 = reinterpret_cast<const uint8_t *>(in_f) + 4ull * n_f + kb;
      const u32 hm = ex.soa_hi_mask;
#pragma unroll
      for (int g = 0; g < KPT / 4; g++) {
        const u32 first = idx_of(g * 4);
        if (nv == (u32)TILE || first + 4u <= nv) {
          const LVec l = *reinterpret_cast<const LVec *>(lo32 + first);
          const u32 h = reinterpret_cast<const HWord *>(hi8 + first)->v;
#pragma unroll
          for (int c = 0; c < 4; c++) keys[g * 4 + c] = (K)((u64)l.v[c] | ((u64)((h >> (8 * c)) & hm) << 32));
        } else {
#pragma unroll
          for (int c = 0; c < 4; c++)
            if (first + (u32)c < nv) keys[g * 4 + c] = (K)((u64)lo32[first + c] | ((u64)((u32)hi8[first + c] & hm) << 32));
        }
      }
      return;
    }
    const K *base = in_f + kb;
#pragma unroll
    for (int g = 0; g < KPT / VEC; g++) {
      const u32 first = idx_of(g * VEC);
      if (nv == (u32)TILE || first + (u32)VEC <= nv) {
        const KVec q = *reinterpret_cast<const KVec *>(base + first);
#pragma unroll
        for (int c = 0; c < VEC; c++) keys[g * VEC + c] = q.v[c];
      } else {
#pragma unroll
        for (int c = 0; c < VEC; c++) if (first + (u32)c < nv) keys[g * VEC + c] = base[first + c];
      }
    }
  };

  // PIPE: a tile in the form it has in memory -- SOA: per group of four keys four low words + one word of high bytes; u32: the words
  static_assert(!PIPE || SOA || sizeof(K) == 4, "the pipelined fetch holds 5-byte or 4-byte keys");
  constexpr int RAWN = PIPE ? (SOA ? KPT + KPT / 4 : KPT) : 1;
  u32 raw[RAWN];
#pragma unroll
  for (int i = 0; i < RAWN; i++) raw[i] = 0u;
  auto fetch_raw = [&](u64 kb, u32 nv) __attribute__((always_inline)) {
    if constexpr (PIPE && SOA) {
      struct __attribute__((aligned(4))) LVec { u32 v[4]; };
      struct __attribute__((packed, aligned(1))) HWord { u32 v; };
      const u32 *lo32 = reinterpret_cast<const u32 *>(in_f) + kb;
      const uint8_t *hi8 = reinterpret_cast<const uint8_t *>(in_f) + 4ull * n_f + kb;
#pragma unroll
      for (int g = 0; g < KPT / 4; g++) {
        const u32 first = idx_of(g * 4);
        if (nv == (u32)TILE || first + 4u <= nv) {
          const LVec l = *reinterpret_cast<const LVec *>(lo32 + first);
#pragma unroll
          for (int c = 0; c < 4; c++) raw[g * 5 + c] = l.v[c];
          raw[g * 5 + 4] = reinterpret_cast<const HWord *>(hi8 + first)->v;
        } else {
          u32 h = 0;
#pragma unroll
          for (int c = 0; c < 4; c++)
            if (first + (u32)c < nv) { raw[g * 5 + c] = lo32[first + c]; h |= (u32)hi8[first + c] << (8 * c); }
          raw[g * 5 + 4] = h;
        }
      }
    } else if constexpr (PIPE) {
      const u32 *base = reinterpret_cast<const u32 *>(in_f) + kb;
      struct __attribute__((aligned(4))) WVec { u32 v[4]; };
      static_assert(!PIPE || SOA || KPT % 4 == 0, "four words per load");
#pragma unroll
      for (int g = 0; g < KPT / 4; g++) {
        const u32 first = idx_of(g * 4);
        if (nv == (u32)TILE || first + 4u <= nv) {
          const WVec q = *reinterpret_cast<const WVec *>(base + first);
#pragma unroll
          for (int c = 0; c < 4; c++) raw[g * 4 + c] = q.v[c];
        } else {
#pragma unroll
          for (int c = 0; c < 4; c++) if (first + (u32)c < nv) raw[g * 4 + c] = base[first + c];
        }
      }
    }
  };
  auto assemble = [&]() __attribute__((always_inline)) {
    if constexpr (PIPE && SOA) {
      const u32 hm = ex.soa_hi_mask;
#pragma unroll
      for (int g = 0; g < KPT / 4; g++)
#pragma unroll
        for (int c = 0; c < 4; c++) {
          if constexpr (NARROW) narrow_to(g * 4 + c, (raw[g * 5 + 4] >> (8 * c)) & hm, raw[g * 5 + c]);
          else                  keys[g * 4 + c] = (K)((u64)raw[g * 5 + c] | ((u64)((raw[g * 5 + 4] >> (8 * c)) & hm) << 32));
        }
    } else if constexpr (PIPE) {
#pragma unroll
      for (int j = 0; j < KPT; j++) keys[j] = (K)raw[j];
    }
  };

  // STAGGER (round 6; the 5-byte first pass): the persistent workgroups start in ex.stagger_groups groups, group g a g/P-th of a
  // tile's time behind group 0, and stay apart -- nothing but the look-back couples them, and it only asks that earlier tiles are not
  // behind.  Started together the ~256 workgroups run in step: a tile's walkers then find nothing but aggregates among their
  // predecessors and the inclusive prefixes spread from the oldest tile on; apart, the tiles of the groups ahead have their prefixes
  // out.  The first tiles are handed out statically in the order in which they will be processed (burst i * P + g = iteration i of
  // group g; a ticket taken while another group sleeps would put a LATER tile in front of its predecessors: measured, +9 %), the
  // tickets continue behind them.  Measured (profiles/r06_ab_runs.txt, r06x_rb8b): first pass 0.453 -> 0.444 ms per launch.
  // OPT-IN (MGC_PASS_STAGGER=8), not the default: with tickets a workgroup that is not resident yet holds no tile, so the walkers only
  // ever wait for workgroups that run; a static hand-out gives tiles to workgroups that may still wait for a CU -- another process or
  // session holding part of the device -- and the running ones would spin for them until the spin limit (MGC_ETIMEOUT).
  const bool stag = ex.stagger_groups > 1u && gridDim.x % (8u * ex.stagger_groups) == 0u;
  u32 st_g = 0, st_r = 0, st_w = 0, tk_off = 0;
  if (stag) {
    st_g = (blockIdx.x >> 3) % ex.stagger_groups;          // (consecutive workgroups go to the eight XCDs in turn: every group on all of them)
    st_r = ((blockIdx.x >> 3) / ex.stagger_groups) * 8u + (blockIdx.x & 7u);
    st_w = gridDim.x / ex.stagger_groups;
    tk_off = (PIPE ? 3u : 2u) * gridDim.x;
    if (st_g) {
      const u64 c0 = __builtin_readcyclecounter(), want = (u64)st_g * ex.stagger_cycles;
      while (__builtin_readcyclecounter() - c0 < want) __builtin_amdgcn_s_sleep(16);
    }
  }
  if (tid == 0) s_tmp[32] = stag ? st_g * st_w + st_r : atomicAdd(ticket, 1u);
  __syncthreads();
  u64 tile = s_tmp[32];
  announce(tile, 0);
  __syncthreads();
  u64 kb = 0; u32 nv = 0;
  u64 tile1 = 0, kb1 = 0; u32 nv1 = 0;                    // PIPE: the tile after the current one (its keys in flight / in raw[])
  // BATCH: file and tile number inside it of the current tile, of tile1 and of `next` (the same in all lanes: scalar registers)
  u32 fi = 0, lt = 0, fi1 = 0, lt1 = 0, nfi = 0, nlt = 0;
  auto info_file = [&](int slot, u32 &f, u32 &l) __attribute__((always_inline)) {
    if constexpr (BATCH) { f = __builtin_amdgcn_readfirstlane(s_tmp[40 + 2 * slot]); l = __builtin_amdgcn_readfirstlane(s_tmp[41 + 2 * slot]); }
  };
  if constexpr (!PIPE) {
    if (tile < total_tiles) { kb = s_info[0]; nv = (u32)s_info[1]; info_file(0, fi, lt); fetch_from(fi); fetch(kb, nv); }
  } else {
    if (tile < total_tiles) { kb = s_info[0]; nv = (u32)s_info[1]; info_file(0, fi, lt); fetch_from(fi); fetch_raw(kb, nv); assemble(); }
    if (tid == 0) s_tmp[33] = stag ? (ex.stagger_groups + st_g) * st_w + st_r : atomicAdd(ticket, 1u);
    __syncthreads();
    tile1 = s_tmp[33];
    announce(tile1, 1);
    __syncthreads();
    if (tile1 < total_tiles) { kb1 = s_info[2]; nv1 = (u32)s_info[3]; info_file(1, fi1, lt1); fetch_from(fi1); fetch_raw(kb1, nv1); }
    __syncthreads();                                      // (s_tmp[33] and s_info[2..3] are written again at the top of the loop)
  }
  // the ticket of the tile after those (from now on taken in the shadow of the look-back, below)
  if (tid == 0) s_tmp[34] = stag ? ((PIPE ? 2u : 1u) * ex.stagger_groups + st_g) * st_w + st_r : atomicAdd(ticket, 1u);

  u64 ph[8] = {0, 0, 0, 0, 0, 0, 0, 0}, t0 = 0;
#define PK_STAMP(i) do { if (DBG) { const u64 t = __builtin_readcyclecounter(); ph[i] += t - t0; t0 = t; } } while (0)
  while (tile < total_tiles) {
    if (DBG) t0 = __builtin_readcyclecounter();
    tid = tid0;
    asm volatile("" : "+v"(tid));                         // keeps the unrolled body's LDS addresses out of the loop preheader
    lane = tid & 63u; w = tid >> 6;
    const bool walker = tid < (u32)G;
    // what belongs to the current tile's file (BATCH: from its descriptor; the row number of the look-back is the tile's number in the file)
    typename GroupOut<K, NARROW>::type *out_c = out;
    const u64 *gbase_c = gbase;
    u64 *status_c = status;
    u64 row = tile;
    if constexpr (BATCH) {
      out_c = reinterpret_cast<typename GroupOut<K, NARROW>::type *>(bfiles[fi].out);
      gbase_c = bfiles[fi].gbase; status_c = bfiles[fi].status; row = lt;
    }
    if (tid < (u32)R) s_hist[tid] = 0;
    __syncthreads();                                      // (A)
    const u64 next = s_tmp[34];
    announce(next, 1);                                    // read after (C)
    PK_STAMP(0);

    // ---- rank: position among the tile's keys of the same digit, in arrival order ----
    u32 ranks[KPT / 2];
    u32 dgs[HPCD ? KPT / 2 : 1];                          // HPCD: the digits stay in registers for the exchange (one table read less per key)
#pragma unroll
    for (int j = 0; j < KPT; j++) {
      u32 r = 0, d = 0;
      if (idx_of(j) < nv) {
        if constexpr (NARROW) { if constexpr (!PIPE) narrow_to(j, (u32)((u64)keys[j] >> 32), (u32)(u64)keys[j]); d = dig_of(j); }
        else d = dig(keys[j]);
        r = atomicAdd(&s_hist[d], 1u);
      }
      if (j & 1) ranks[j / 2] |= r << 16;
      else       ranks[j / 2]  = r;
      if constexpr (HPCD) { if (j & 1) dgs[j / 2] |= d << 16; else dgs[j / 2] = d; }
    }
    __syncthreads();                                      // (B)
    PK_STAMP(1);

    const u32 count = (tid < (u32)R) ? s_hist[tid] : 0u;
    u32 tile_total;
    const u32 excl = block_excl_scan<BLOCK, u32>(count, s_tmp, &tile_total);
    if (tid < (u32)R) { s_cnt[tid] = count; s_dbase[tid] = excl; }
    __syncthreads();                                      // (C)
    if constexpr (NARROW) {
      // the exchange takes its digits, its counter addresses and its in-tile tests afresh: kept from the ranking they are a vector
      // register (the address) and a scalar pair (the test) per key, held across the scan -- with 20 and 24 keys per thread that spills
      asm volatile("" : "+v"(tid));
      lane = tid & 63u; w = tid >> 6;
#pragma unroll
      for (int j = 0; j < KPT / DPR; j++) asm volatile("" : "+v"(dgp[j]));
    }

    u64 *mine = status_c + row * (u64)G + tid;
    u32 c0 = 0, c1 = 0;
    if (walker) {
      c0 = s_cnt[2 * tid]; c1 = s_cnt[2 * tid + 1];
      const u32 fl = (row == 0) ? 2u : 1u;
      status_store(mine, st_pack(fl, c0, fl, c1));
    }
#pragma unroll
    for (int j = 0; j < KPT; j++) {
      if (idx_of(j) < nv) {
        u32 d;
        if constexpr (HPCD) d = (j & 1) ? (dgs[j / 2] >> 16) : (dgs[j / 2] & 0xFFFFu);
        else if constexpr (NARROW) d = dig_of(j);
        else d = dig(keys[j]);
        const u32 r = (j & 1) ? (ranks[j / 2] >> 16) : (ranks[j / 2] & 0xFFFFu);
        if constexpr (NARROW) { const u32 pos = s_dbase[d] + r; s_words[pos] = wd[j]; s_dig[pos] = (DT)d; }
        else s_keys[s_dbase[d] + r] = keys[j];
      }
    }
    u64 nkb = 0; u32 nnv = 0;
    if (next < total_tiles) { nkb = s_info[2]; nnv = (u32)s_info[3]; info_file(1, nfi, nlt); fetch_from(nfi); }
    __syncthreads();                                      // (D) keys live in LDS only
    PK_STAMP(2);

    // Look-back.  Persistent workgroups run in step, so the ~256 tiles in flight reach this point together
    // and the inclusive prefixes can only spread from the oldest tile on: a walker that covers WALK
    // predecessors per round trip sees the frontier move ~2*WALK tiles per round trip.  (Measured: holding
    // the key fetch back, or issuing the status loads ahead of it, does not shorten the walk.)
    u32 p0 = 0, p1 = 0;
    bool done = (row == 0);
    u64  wt = row ? row - 1 : 0;
    u32  spins = 0;
    u64  gv[WALK];
    auto issue = [&]() __attribute__((always_inline)) {
#pragma unroll
      for (int i = 0; i < WALK; i++)
        gv[i] = (wt >= (u64)i) ? status_load(status_c + (wt - i) * (u64)G + tid) : st_pack(2, 0, 2, 0);
    };
    auto consume = [&]() __attribute__((always_inline)) {
      u32 used = 0;
      bool open = true;
#pragma unroll
      for (int i = 0; i < WALK; i++) {
        const u32 lo = (u32)gv[i], hi = (u32)(gv[i] >> 32);
        const u32 f = lo >> 30;
        open = open && !done && (f != 0);
        if (open) {
          p0 += lo & 0x3FFFFFFFu; p1 += hi & 0x3FFFFFFFu;
          if (f == 2) done = true;
          used++;
        }
      }
      wt -= (used <= wt) ? used : wt;
      if (used == 0) {
        if (++spins > RS_SPIN_LIMIT) { atomicExch(error_flag, 1u); done = true; }
        else __builtin_amdgcn_s_sleep(1);
      }
    };
    if (!walker) {
      // the last thread asks for the ticket of the tile after `next` here and hands it over before (E) (read behind the next (A)): its
      // wave's wait for the answer -- vmcnt is in order: also for what the wave has in flight -- lies in the shadow of the look-back
      // (until round 6 tid 0 asked at the top of the loop and the whole workgroup waited at (A) behind that wave's write-out stores and,
      // PIPE, the prefetch it had just issued: ~2 K cycles per tile)
      u32 tk_pre = 0;
      if (tid == (u32)BLOCK - 1u) tk_pre = atomicAdd(ticket, 1u) + tk_off;
      if constexpr (!PIPE) { if (next < total_tiles) fetch(nkb, nnv); }
      // the waves that do not walk would only wait now: they count the other digit of the tile's keys (in LDS, in digit
      // order since the exchange) -- LDS work in the shadow of the look-back
      if constexpr (HIST2) {
        for (u32 i = tid - (u32)G; i < nv; i += (u32)(BLOCK - G)) {
          if constexpr (NARROW) atomicAdd(&s_h2[(s_words[i] >> shift2w) & ex.mask2], 1u);
          else                  atomicAdd(&s_h2[dig2(s_keys[i])], 1u);
        }
      }
      if (tid == (u32)BLOCK - 1u) s_tmp[34] = tk_pre;
    } else {
      while (!done) { issue(); consume(); }
      if (row != 0) status_store(mine, st_pack(2, p0 + c0, 2, p1 + c1));
      s_gbase[2 * tid]     = gbase_c[2 * tid]     + (u64)p0 - (u64)s_dbase[2 * tid];
      s_gbase[2 * tid + 1] = gbase_c[2 * tid + 1] + (u64)p1 - (u64)s_dbase[2 * tid + 1];
      if constexpr (!PIPE) { if (next < total_tiles) fetch(nkb, nnv); }
    }
    __syncthreads();                                      // (E)
    PK_STAMP(3);
    if constexpr (PIPE) {
      // the tile fetched a whole tile ago leaves raw[] for keys[] (nothing newer is in flight when the wait for it runs: the
      // write-out's stores come AFTER this point), and the tile after it is asked for
      if (tile1 < total_tiles) assemble();
      if (PIPE == 1 && next < total_tiles) fetch_raw(nkb, nnv);
    }

#pragma unroll
    for (int j = 0; j < KPT; j++) {
      const u32 i = (u32)j * BLOCK + tid;
      if (i < nv) {
        if constexpr (NARROW) out_c[s_gbase[s_dig[i]] + (u64)i] = s_words[i];
        else {
          const K   key = s_keys[i];
          const u32 d   = dig(key);
          out_c[s_gbase[d] + (u64)i] = key;
        }
      }
    }
    PK_STAMP(4);
    if constexpr (PIPE == 2) { if (next < total_tiles) fetch_raw(nkb, nnv); }
    __syncthreads();                                      // (F)
    PK_STAMP(5);
    if constexpr (BATCH && HIST2) {
      // the current tile is the workgroup's last of its file (or its last): the other digit's counts go to that file's histogram.
      // Behind (F) every count of the tile is in; a thread clears the counters it has read, and the next counts come behind (A)..(D).
      const bool leaves = PIPE ? (tile1 >= total_tiles || fi1 != fi) : (next >= total_tiles || nfi != fi);
      if (leaves) {
        u64 *gh = bfiles[fi].ghist2;
        for (u32 i = tid0; i < (u32)RS_MAX_RADIX; i += BLOCK) { const u32 c = s_h2[i]; if (c) { atomicAdd(&gh[i], (u64)c); s_h2[i] = 0; } }
      }
    }
    if constexpr (PIPE) { tile = tile1; kb = kb1; nv = nv1; tile1 = next; kb1 = nkb; nv1 = nnv; fi = fi1; lt = lt1; fi1 = nfi; lt1 = nlt; }
    else                { tile = next; kb = nkb; nv = nnv; fi = nfi; lt = nlt; }
    if (DBG) ph[7]++;
  }
  if (DBG && tid0 == 0 && blockIdx.x < 64)
    for (int i = 0; i < 8; i++) dbg[blockIdx.x * 8 + i] = ph[i];
#undef PK_STAMP
  (void)kb;
  if constexpr (HIST2 && !BATCH) {
    __syncthreads();
    for (u32 i = tid0; i < (u32)RS_MAX_RADIX; i += BLOCK) { const u32 c = s_h2[i]; if (c) atomicAdd(&ex.ghist2[i], (u64)c); }
  }
  (void)fi; (void)lt; (void)fi1; (void)lt1; (void)nfi; (void)nlt; (void)af;
}

struct NarrowPrep { unsigned char bits_a[256]; unsigned char on[256]; };   // per bucket: bits of its first (high) digit, narrowed at all

// ---- host side ---------------------------------------------------------------

void make_sort_plan(uint32_t begin_bit, uint32_t end_bit, SortPlan *plan) {
  memset(plan, 0, sizeof(*plan));
  // the fastest measured combination on MI355X (profiles/r01*, DESIGN_HISTORY.md): nine-bit digits, one 1024-thread workgroup
  // per CU with 16 keys per thread (8 for 16-byte keys), LDS-mask ranking, window look-back after the exchange.  The other
  // shapes (eight-bit digits, 512-thread workgroups, ballot ranking, serial and pipelined look-back, the classic
  // histogram / scan / scatter form) were measured in rounds 1-2 and removed in round 5.
  plan->radix_bits = 9;
  plan->block      = 1024;
  plan->kpt        = 16;
  plan->tile       = plan->block * plan->kpt;
  plan->mode       = 0;                                                 // 0 stable sort; the caller sets 3 for grouping passes
  const uint32_t rb = plan->radix_bits;
  const uint32_t nbits = (end_bit > begin_bit) ? end_bit - begin_bit : 0;
  uint32_t passes = (nbits + rb - 1) / rb;
  if (passes > RS_MAX_PASSES) passes = RS_MAX_PASSES;
  plan->num_passes = passes;
  uint32_t bit = begin_bit;
  for (uint32_t p = 0; p < passes; p++) {
    uint32_t b = nbits / passes + ((p < nbits % passes) ? 1u : 0u);
    plan->pass_shift[p] = bit;
    plan->pass_bits[p]  = b;
    bit += b;
  }
}

void make_hpc_group_plan(uint32_t low_bit, uint32_t passes, SortPlan *plan) {
  make_sort_plan(0, 18, plan);                       // tile shape, look-back flavour, env overrides
  plan->radix_bits = 9;                              // 243 of the 512 bins are used
  plan->mode = 3;
  plan->hpc = 1;
  plan->num_passes = passes;
  for (uint32_t p = 0; p < passes; p++) { plan->pass_shift[p] = low_bit + 10 * p; plan->pass_bits[p] = 10; }
}

// `compress`, a bucket of 14..45 M k-mers on the distinct-sized count: the HIGH digit a dense rank of five bases (243 values), the LOW
// one the plain eight bits of the four bases below them (81 of 256 patterns occur): 19683 occupied sub-buckets instead of 59049
void make_hpc_mixed_plan(uint32_t low_bit, SortPlan *plan) {
  make_hpc_group_plan(low_bit, 2, plan);
  plan->hpc = 2;
  plan->pass_shift[0] = low_bit;     plan->pass_bits[0] = 8;
  plan->pass_shift[1] = low_bit + 8; plan->pass_bits[1] = 10;
}

// the `mask` argument of a pass's kernels (hpc == 2: only the high digit of the two is a dense rank)
static inline u32 plan_mask(const SortPlan &plan, uint32_t p) {
  return (plan.hpc == 1 || (plan.hpc == 2 && p == 1)) ? HPC_DIGIT_MASK : (1u << plan.pass_bits[p]) - 1u;
}

static inline uint64_t max_tiles_for(uint64_t n) { return (n + 4095) / 4096 + 1; }   // tile >= 4096 keys

size_t sort_workspace_bytes(uint64_t n) {
  // header + the larger of {look-back granules (one pass at a time), classic tile_hist + tile_offs}
  const uint64_t t = max_tiles_for(n);
  // + grouping mode: up to RS_MAX_RADIX + 1 extra (partial) tiles of granules and the region table
  return sizeof(SortHeader) + 1024 + (size_t)t * RS_MAX_RADIX * (sizeof(uint32_t) + sizeof(uint64_t)) +
         (size_t)(RS_MAX_RADIX + 2) * (RS_MAX_RADIX / 2) * sizeof(uint64_t) + (size_t)(RS_MAX_RADIX + 2) * 16;
}

static int device_cu_count() {
  static int cus = 0;
  if (!cus) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0)
      cus = 256;
  }
  return cus;
}

// digit histograms + exclusive digit bases of a file's passes into `hdr` (tickets zeroed)
template <typename K>
static hipError_t group_prepare(const K *src, uint64_t n, const SortPlan &plan, SortHeader *hdr, hipStream_t st) {
  MGC_CHECK(hipMemsetAsync(hdr, 0, sizeof(SortHeader), st));
  PassList pl;
  pl.n = plan.num_passes;
  for (uint32_t p = 0; p < plan.num_passes; p++) {
    pl.shift[p] = plan.pass_shift[p];
    pl.mask[p]  = plan_mask(plan, p);
  }
  launch_radix_hist<K>(src, (u64)n, pl, &hdr->ghist[0][0], st);
  MGC_CHECK(hipGetLastError());
  hipLaunchKernelGGL(radix_digit_scan_kernel, dim3(plan.num_passes), dim3(RS_MAX_RADIX), 0, st,
                     &hdr->ghist[0][0], &hdr->gbase[0][0]);
  return hipGetLastError();
}

// ---- one launch of radix_group_kernel: what it takes (GroupPass), which instantiation (GroupInst, mgc_group_route.hpp) ----
struct GroupPass {
  const void *in; void *out;                 // K keys in; K keys out (a NARROW pass: u32 words)
  u64 n; u32 shift, mask;
  const u64 *gbase; u64 *status; u32 *ticket; u32 *d_error;
  u64 tiles_plain;                           // tiles of n keys without region cuts
  u64 *region_start; u32 *region_tiles;      // the regions a second pass's tiles are cut at; null on a first pass
  GroupExtra ex;
  u64 *dbg;                                  // DBG: where the cycle sums go
  u64 tile_bound;                            // no tile index reaches this: the grid is min(tile_bound, resident workgroups)
  hipStream_t st;
  // a batched instantiation (GroupInst::batch): the files' descriptors on the device and their number; shift, mask, ticket, d_error,
  // ex, tile_bound and st are the launch's, everything else is in the descriptors
  const GroupBatchFile *bfiles = nullptr; u32 nbf = 0;
};
static hipError_t launch_group_pass(const GroupInst &inst, const GroupPass &p);   // (the table, below the tile constants)

template <typename K> constexpr GroupKey group_key_of();
template <> constexpr GroupKey group_key_of<u64>()  { return GROUP_U64; }
template <> constexpr GroupKey group_key_of<u32>()  { return GROUP_U32; }
template <> constexpr GroupKey group_key_of<K128>() { return GROUP_K128; }
template <> constexpr GroupKey group_key_of<K96>()  { return GROUP_K96; }

// LB 2: packed granules (n < 2^30); LB 3: wide granules
template <typename K, int KPT, int LB>
static hipError_t run_passes(void *d_keys, void *d_alt, uint64_t n, const SortPlan &plan, void *d_ws,
                             uint32_t *d_error, int *result_in_alt, hipStream_t st, hipEvent_t *pass_events) {
  constexpr int RB = 9, BLOCK = 1024;
  using SM = RadixSmem<K, RB, BLOCK, KPT, LB>;
  constexpr int R = 1 << RB, TILE = BLOCK * KPT;
  SortHeader *hdr = reinterpret_cast<SortHeader *>(d_ws);
  unsigned char *body = reinterpret_cast<unsigned char *>(d_ws) + ((sizeof(SortHeader) + 255) / 256) * 256;
  const uint64_t num_tiles = (n + TILE - 1) / TILE;

  K *src = reinterpret_cast<K *>(d_keys), *dst = reinterpret_cast<K *>(d_alt);
  int in_alt = 0;
  u64 *status = reinterpret_cast<u64 *>(body);
  MGC_CHECK(group_prepare<K>((const K *)src, n, plan, hdr, st));

  if (plan.mode != 3) {
    static bool attr_done = false;
    if (!attr_done) {
      (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&radix_scatter_kernel<K, RB, BLOCK, KPT, LB>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)SM::BYTES);
      attr_done = true;
    }
    const size_t status_bytes = (size_t)num_tiles * (LB == 3 ? R : R / 2) * sizeof(u64);
    for (uint32_t p = 0; p < plan.num_passes; p++) {
      MGC_CHECK(hipMemsetAsync(status, 0, status_bytes, st));
      if (pass_events) MGC_CHECK(hipEventRecord(pass_events[2 * p], st));
      hipLaunchKernelGGL((radix_scatter_kernel<K, RB, BLOCK, KPT, LB>), dim3((uint32_t)num_tiles),
                         dim3(BLOCK), SM::BYTES, st, (const K *)src, dst, (u64)n, plan.pass_shift[p],
                         plan_mask(plan, p), &hdr->gbase[p][0], status, &hdr->ticket[p], d_error);
      MGC_CHECK(hipGetLastError());
      if (pass_events) MGC_CHECK(hipEventRecord(pass_events[2 * p + 1], st));
      K *t = src; src = dst; dst = t; in_alt ^= 1;
    }
  } else {
    // ---- grouping passes (finish path): see radix_group_kernel ----
    constexpr GroupInst inst = group_pick_sorted(group_key_of<K>());
    static_assert(group_tile(inst) == (uint64_t)TILE, "the sort's tile");
    const uint64_t max_tiles = num_tiles + RS_MAX_RADIX + 1;          // region-aligned tiles: one partial tile per region
    const size_t status_bytes = (size_t)max_tiles * (R / 2) * sizeof(u64);
    u64 *region_start = reinterpret_cast<u64 *>(body + ((status_bytes + 255) / 256) * 256);
    u32 *region_tiles = reinterpret_cast<u32 *>(region_start + RS_MAX_RADIX + 1);
    for (uint32_t p = 0; p < plan.num_passes; p++) {
      if (p == 1) {
        hipLaunchKernelGGL(group_regions_kernel, dim3(1), dim3(RS_MAX_RADIX), 0, st, &hdr->gbase[0][0], (u64)n, (u32)TILE,
                           region_start, region_tiles);
        MGC_CHECK(hipGetLastError());
      }
      MGC_CHECK(hipMemsetAsync(status, 0, status_bytes, st));
      if (pass_events) MGC_CHECK(hipEventRecord(pass_events[2 * p], st));
      const GroupPass gp{src, dst, (u64)n, plan.pass_shift[p], plan_mask(plan, p), &hdr->gbase[p][0], status, &hdr->ticket[p], d_error,
                         (u64)num_tiles, p ? region_start : nullptr, p ? region_tiles : nullptr, GroupExtra{0u, 0u, 0u, nullptr}, nullptr,
                         (u64)(p ? max_tiles : num_tiles), st};
      MGC_CHECK(launch_group_pass(inst, gp));
      if (pass_events) MGC_CHECK(hipEventRecord(pass_events[2 * p + 1], st));
      K *t = src; src = dst; dst = t; in_alt ^= 1;
    }
  }
  *result_in_alt = in_alt;
  return hipSuccess;
}

// ---- two grouping passes with narrowed keys (the finish path of k-mers that leave <= 32 bits below their first digit) ----
// Sub-bucket v = (digit of pass 1 : digit of pass 0).  Pass 1's tiles never mix two pass-0 digits (regions), its output is
// ordered by (pass-1 digit, tile), so sub-bucket v starts at  gbase1[d1] + the inclusive prefix of d1 at the last tile
// before region d0  -- which is exactly what the look-back granules of pass 1 hold once the pass is over: the boundaries
// come for free, no key has to be looked at (the keys do not even hold d0 any more).
__global__ void narrow_bounds_kernel(const u64 *__restrict__ status, const u32 *__restrict__ region_tiles,
                                     const u64 *__restrict__ gbase1, u64 n, u32 b0, u64 ng, u64 *__restrict__ starts,
                                     u32 granules /* per tile: half the digits of the pass's instantiation */) {
  const u64 v = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (v > ng) return;
  if (v == ng) { starts[v] = n; return; }
  u32 d1 = (u32)(v >> b0), d0 = (u32)v & ((1u << b0) - 1u);
  // dense-rank digits (`compress`) live in ten-bit fields but stay below 364: nothing lies at or beyond a digit >= RS_MAX_RADIX
  if (d1 >= (u32)RS_MAX_RADIX) { starts[v] = n; return; }
  if (d0 > (u32)RS_MAX_RADIX) d0 = RS_MAX_RADIX;
  const u32 tiles_before = region_tiles[d0];
  u64 before = 0;
  if (tiles_before) {
    if ((d1 >> 1) >= granules) { starts[v] = n; return; }   // (a digit the pass's instantiation does not have: nothing lies there)
    const u64 g = status[(u64)(tiles_before - 1) * granules + (d1 >> 1)];
    before = (u64)(((d1 & 1u) ? (u32)(g >> 32) : (u32)g) & 0x3FFFFFFFu);
  }
  starts[v] = gbase1[d1] + before;
}

bool sort_plan_narrows(const SortPlan &plan, uint64_t n, uint32_t key_words, bool on) {
  return on && key_words == 1 && plan.mode == 3 && !plan.hpc && plan.num_passes == 2 && plan.radix_bits == 9 && n > 0 && n < (1ull << 30) &&
         plan.pass_shift[1] == plan.pass_shift[0] + plan.pass_bits[0] &&
         plan.pass_shift[0] + std::max(plan.pass_bits[0], plan.pass_bits[1]) <= 32;     // whichever digit goes first, the rest fits a word
}

// ---- the small per-file steps of the high-digit-first form, batched over all files (a launch per file and step costs more idle
// time than the steps themselves: ~8 us each, ten of them per file) ----

// one workgroup per file: header cleared, histogram of the file's top bits_a[f] bits from the 512 fine counts, its exclusive scan
// fb: fine holds 2^fb counts per bucket (the fifteen-bit histogram of 2^(15 - fb) buckets: 9 for the 64 files, 8 / 7 for the 128 / 256
// buckets of a sharded count); bits_a[f] <= fb
__global__ __launch_bounds__(RS_MAX_RADIX)
void narrow_prepare_kernel(const u64 *__restrict__ fine, NarrowPrep prep, unsigned char *__restrict__ hdrs, u32 hdr_stride, u32 fb) {
  __shared__ u64 s_f[RS_MAX_RADIX];
  __shared__ u64 s_tmp[RS_MAX_RADIX / 64 + 1];
  const u32 f = blockIdx.x, x = threadIdx.x;
  if (!prep.on[f]) return;
  SortHeader *hdr = reinterpret_cast<SortHeader *>(hdrs + (size_t)f * hdr_stride);
  u32 *w = reinterpret_cast<u32 *>(hdr);
  for (u32 i = x; i < sizeof(SortHeader) / 4; i += RS_MAX_RADIX) w[i] = 0;
  s_f[x] = (x < (1u << fb)) ? fine[((size_t)f << fb) + x] : 0ull;
  __syncthreads();
  const u32 bits = prep.bits_a[f], span = 1u << (fb - bits);
  u64 c = 0;
  if (x < (1u << bits)) for (u32 i = 0; i < span; i++) c += s_f[x * span + i];
  u64 total;
  const u64 e = block_excl_scan<RS_MAX_RADIX, u64>(c, s_tmp, &total);
  hdr->ghist[0][x] = c;
  hdr->gbase[0][x] = e;
}

// between the two passes: exclusive scan of the second digit's histogram (taken by the first pass) + the region table
__global__ __launch_bounds__(RS_MAX_RADIX)
void narrow_mid_kernel(SortHeader *__restrict__ hdr, u64 n, u32 tile, u64 *__restrict__ region_start, u32 *__restrict__ region_tiles) {
  __shared__ u64 s_tmp[RS_MAX_RADIX / 64 + 1];
  __shared__ u32 s_tmp32[RS_MAX_RADIX / 64 + 1];
  const u32 r = threadIdx.x;
  u64 total;
  const u64 e = block_excl_scan<RS_MAX_RADIX, u64>(hdr->ghist[1][r], s_tmp, &total);
  hdr->gbase[1][r] = e;
  const u64 a = hdr->gbase[0][r], b = (r + 1 < RS_MAX_RADIX) ? hdr->gbase[0][r + 1] : n;
  const u32 nt = (u32)((b - a + tile - 1) / tile);
  u32 tt;
  const u32 et = block_excl_scan<RS_MAX_RADIX, u32>(nt, s_tmp32, &tt);
  region_start[r] = a;
  region_tiles[r] = et;
  if (r == 0) { region_start[RS_MAX_RADIX] = n; region_tiles[RS_MAX_RADIX] = tt; }
}

// The same for the files of a batch (mgc_device.h, GroupBatch): one workgroup per file -- p1 / p2: the descriptors of the first / second
// pass's launch -- and the workgroup that finishes LAST turns the files' second-pass tile counts into their exclusive prefix
// (GroupBatchFile::tile0 of p2; entry [nbf] the total): the number a batched second pass needs and only the device knows.
__global__ __launch_bounds__(RS_MAX_RADIX)
void narrow_mid_batch_kernel(const GroupBatchFile *__restrict__ p1, GroupBatchFile *__restrict__ p2, u32 nbf, u32 tile, u32 *__restrict__ arrived) {
  __shared__ u64 s_tmp[RS_MAX_RADIX / 64 + 1];
  __shared__ u32 s_tmp32[RS_MAX_RADIX / 64 + 1];
  __shared__ u32 s_last;
  const u32 r = threadIdx.x, f = blockIdx.x;
  const u64 n = p2[f].n;
  const u64 *ghist1 = p1[f].ghist2, *gbase0 = p1[f].gbase;
  u64 *gbase1 = p2[f].gbase, *region_start = p2[f].region_start;
  u32 *region_tiles = p2[f].region_tiles;
  u64 total;
  const u64 e = block_excl_scan<RS_MAX_RADIX, u64>(ghist1[r], s_tmp, &total);
  gbase1[r] = e;
  const u64 a = gbase0[r], b = (r + 1 < RS_MAX_RADIX) ? gbase0[r + 1] : n;
  const u32 nt = (u32)((b - a + tile - 1) / tile);
  u32 tt;
  const u32 et = block_excl_scan<RS_MAX_RADIX, u32>(nt, s_tmp32, &tt);
  region_start[r] = a;
  region_tiles[r] = et;
  if (r == 0) {
    region_start[RS_MAX_RADIX] = n; region_tiles[RS_MAX_RADIX] = tt;
    status_store(&p2[f].tiles, (u64)tt);
    __threadfence();
    s_last = (atomicAdd(arrived, 1u) == nbf - 1u) ? 1u : 0u;
  }
  __syncthreads();
  if (s_last && r == 0) {
    __threadfence();
    u64 at = 0;
    for (u32 i = 0; i < nbf; i++) { p2[i].tile0 = at; at += status_load(&p2[i].tiles); }
    p2[nbf].tile0 = at;
  }
}

// narrow_bounds_kernel for the files of a batch: the file in blockIdx.y, what is the file's from its second-pass descriptor
__global__ void narrow_bounds_batch_kernel(const GroupBatchFile *__restrict__ p2, u32 b0, u64 ng, u32 granules) {
  const GroupBatchFile &d = p2[blockIdx.y];
  const u64 *status = d.status, *gbase1 = d.gbase;
  const u32 *region_tiles = d.region_tiles;
  u64 *starts = d.sub_starts;
  const u64 n = d.n;
  const u64 v = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (v > ng) return;
  if (v == ng) { starts[v] = n; return; }
  u32 d1 = (u32)(v >> b0), d0 = (u32)v & ((1u << b0) - 1u);
  if (d1 >= (u32)RS_MAX_RADIX) { starts[v] = n; return; }
  if (d0 > (u32)RS_MAX_RADIX) d0 = RS_MAX_RADIX;
  const u32 tiles_before = region_tiles[d0];
  u64 before = 0;
  if (tiles_before) {
    if ((d1 >> 1) >= granules) { starts[v] = n; return; }   // (a digit the pass's instantiation does not have: nothing lies there)
    const u64 g = status[(u64)(tiles_before - 1) * granules + (d1 >> 1)];
    before = (u64)(((d1 & 1u) ? (u32)(g >> 32) : (u32)g) & 0x3FFFFFFFu);
  }
  starts[v] = gbase1[d1] + before;
}

// per-file scratch of the batched form: [status of pass A][status of pass B][region table]
// Keys per tile of the first / second pass (launch_group_narrow).  The first pass exchanges 5 or 6 bytes per key (group_xb), so the LDS
// has room for 24576 keys; the register file has it only where the next tile waits in the form it has in memory (PIPE: 30 registers
// for 24 keys of the 5-byte layout) -- the forms that fetch whole 8-byte keys inside the look-back (MGC_GROUP_PIPE=0, MGC_SOA5=0, the
// owner side of a sharded count) hold 48 registers of them beside the words and spill at 20 and at 24 keys per thread: they keep 16.
#ifndef MGC_NARROW_KPT0
#define MGC_NARROW_KPT0 24                                       // keys per thread of the pipelined first pass (A/B builds: 16, 20)
#endif
constexpr uint64_t NARROW_TILE0 = 16384, NARROW_TILE0P = 1024ull * MGC_NARROW_KPT0, NARROW_TILE1 = 24576;
// a pipelined first-pass tile's time, which the staggered groups share: 31000 cycles measured at 16384 keys (MGC_GROUP_DBG), scaled
constexpr uint32_t NARROW_TILE0_CYCLES = 31000u * MGC_NARROW_KPT0 / 16u;
size_t narrow_scratch_bytes(uint64_t n) {
  static_assert(NARROW_TILE0 <= NARROW_TILE0P, "rows for the smaller of the first pass's tiles");
  const uint64_t tiles0 = (n + NARROW_TILE0 - 1) / NARROW_TILE0, tiles1_max = (n + NARROW_TILE1 - 1) / NARROW_TILE1 + RS_MAX_RADIX + 1;
  return (size_t)(tiles0 + tiles1_max) * (RS_MAX_RADIX / 2) * sizeof(u64) + (size_t)(RS_MAX_RADIX + 2) * 16 + 512;
}

// headers of all files at once (files with on[f] = 0 are skipped); d_hdrs: nb x sort_header_bytes()
hipError_t launch_narrow_prepare(const uint64_t *d_fine, uint32_t nb, const unsigned char *bits_a, const unsigned char *on, void *d_hdrs,
                                 hipStream_t st) {
  if (nb != 64 && nb != 128 && nb != 256) return hipErrorInvalidValue;
  const u32 fb = nb == 64 ? 9u : (nb == 128 ? 8u : 7u);
  NarrowPrep prep;
  memset(&prep, 0, sizeof(prep));
  memcpy(prep.bits_a, bits_a, nb);
  memcpy(prep.on, on, nb);
  for (uint32_t b = 0; b < nb; b++) if (prep.on[b] && prep.bits_a[b] > fb) return hipErrorInvalidValue;
  hipLaunchKernelGGL(narrow_prepare_kernel, dim3(nb), dim3(RS_MAX_RADIX), 0, st, reinterpret_cast<const u64 *>(d_fine), prep,
                     reinterpret_cast<unsigned char *>(d_hdrs), (u32)sort_header_bytes(), fb);
  return hipGetLastError();
}

// ---- the launcher and the table ----
// One instantiation: the dynamic-LDS limit raised once (the tile, plus the rank table where HPCD), the persistent grid of its own
// WG_PER_CU -- 1 for every row of the table, asserted below -- and the launch.
template <typename K, int RB, int KPT, bool DBG, bool NARROW, bool HIST2, bool SOA, int PIPE, int HPCD, bool BATCH>
static hipError_t group_launch_form(const GroupPass &p) {
  constexpr int BLOCK = GROUP_BLOCK;
  using SM = GroupSmem<K, RB, BLOCK, KPT, group_xb<K, RB, NARROW>()>;
  constexpr size_t LDS = SM::BYTES + (HPCD ? GROUP_RANK_TABLE_BYTES : 0);
  static_assert(!BATCH || (!DBG && !HPCD), "the batched forms");
  if (BATCH && (!p.bfiles || !p.nbf)) return hipErrorInvalidValue;
  static const hipError_t raised = hipFuncSetAttribute(reinterpret_cast<const void *>(&radix_group_kernel<K, RB, BLOCK, KPT, DBG, NARROW, HIST2, SOA, PIPE, HPCD, BATCH>),
                                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS);
  (void)raised;
  const u64 resident = (u64)device_cu_count() * SM::WG_PER_CU;
  // (a batched launch: the descriptors go where a per-file launch has its regions, their number where it has its keys' number)
  hipLaunchKernelGGL((radix_group_kernel<K, RB, BLOCK, KPT, DBG, NARROW, HIST2, SOA, PIPE, HPCD, BATCH>), dim3((uint32_t)std::min(p.tile_bound, resident)),
                     dim3(BLOCK), LDS, p.st, reinterpret_cast<const K *>(p.in), reinterpret_cast<typename GroupOut<K, NARROW>::type *>(p.out),
                     BATCH ? (u64)p.nbf : p.n, p.shift, p.mask, p.gbase, p.status, p.ticket, p.d_error, p.tiles_plain,
                     BATCH ? reinterpret_cast<const u64 *>(p.bfiles) : (const u64 *)p.region_start, (const u32 *)p.region_tiles, p.ex, p.dbg);
  return hipGetLastError();
}

// Every instantiation of radix_group_kernel the library holds: K, RB, KPT, DBG, NARROW, HIST2, SOA, PIPE, HPCD, BATCH (the rules that
// pick among them: mgc_group_route.hpp; pinned by tests/test_group_route_host.py)
#define MGC_GROUP_INSTS(X)                                                                                                     \
  /* a narrowed file's first pass: low digit first; high digit first off whole keys / the 5-byte layout / that a tile ahead */ \
  X(u64, 9, 16, false, true, false, false, 0, 0, false)                                                                        \
  X(u64, 9, 16, false, true, true, false, 0, 0, false)                                                                         \
  X(u64, 9, 16, false, true, true, true, 0, 0, false)                                                                          \
  X(u64, 9, MGC_NARROW_KPT0, false, true, true, true, 2, 0, false)                                                             \
  X(u64, 8, MGC_NARROW_KPT0, false, true, true, true, 2, 0, false)                                                             \
  X(u64, 9, 16, true, true, true, false, 0, 0, false)                                                                          \
  X(u64, 9, 16, true, true, true, true, 0, 0, false)                                                                           \
  X(u64, 9, MGC_NARROW_KPT0, true, true, true, true, 2, 0, false)                                                              \
  /* the two pipelined 5-byte first passes and the two second passes over the files of a batch */                              \
  X(u64, 9, MGC_NARROW_KPT0, false, true, true, true, 2, 0, true)                                                              \
  X(u64, 8, MGC_NARROW_KPT0, false, true, true, true, 2, 0, true)                                                              \
  X(u32, 9, 24, false, false, false, false, 0, 0, true)                                                                        \
  X(u32, 8, 24, false, false, false, false, 0, 0, true)                                                                        \
  /* its second pass */                                                                                                        \
  X(u32, 9, 24, false, false, false, false, 0, 0, false)                                                                       \
  X(u32, 8, 24, false, false, false, false, 0, 0, false)                                                                       \
  X(u32, 9, 24, true, false, false, false, 0, 0, false)                                                                        \
  /* whole keys: first (HIST2) and second pass, nine- and eight-bit digits (the nine-bit second passes: launch_radix_sort too) */ \
  X(u64, 9, 16, false, false, true, false, 0, 0, false)                                                                        \
  X(u64, 9, 16, false, false, false, false, 0, 0, false)                                                                       \
  X(u64, 8, 16, false, false, true, false, 0, 0, false)                                                                        \
  X(u64, 8, 16, false, false, false, false, 0, 0, false)                                                                       \
  X(K128, 9, 8, false, false, true, false, 0, 0, false)                                                                        \
  X(K128, 9, 8, false, false, false, false, 0, 0, false)                                                                       \
  X(K128, 8, 8, false, false, true, false, 0, 0, false)                                                                        \
  X(K128, 8, 8, false, false, false, false, 0, 0, false)                                                                       \
  X(K96, 9, 12, false, false, true, false, 0, 0, false)                                                                        \
  X(K96, 9, 12, false, false, false, false, 0, 0, false)                                                                       \
  X(K96, 8, 12, false, false, true, false, 0, 0, false)                                                                        \
  X(K96, 8, 12, false, false, false, false, 0, 0, false)                                                                       \
  /* `compress`: both digits dense ranks (first, second pass); only the high one (first pass) */                              \
  X(u64, 9, 16, false, false, true, false, 0, 1, false)                                                                        \
  X(u64, 9, 16, false, false, false, false, 0, 1, false)                                                                       \
  X(u64, 9, 16, false, false, true, false, 0, 2, false)                                                                        \
  X(K128, 9, 8, false, false, true, false, 0, 1, false)                                                                        \
  X(K128, 9, 8, false, false, false, false, 0, 1, false)                                                                       \
  X(K128, 9, 8, false, false, true, false, 0, 2, false)

// every row: one workgroup per CU (so "the instantiation's own WG_PER_CU" is the grid every launch had), and the LDS bytes the
// picking functions reckon with (the rank table only where it fits) are the kernel's
#define MGC_GROUP_ROW_OK(K, RB, KPT, DBG, NARROW, HIST2, SOA, PIPE, HPCD, BATCH)                                                      \
  static_assert(GroupSmem<K, RB, GROUP_BLOCK, KPT, group_xb<K, RB, NARROW>()>::WG_PER_CU == 1, "one workgroup per CU");        \
  static_assert(GroupSmem<K, RB, GROUP_BLOCK, KPT, group_xb<K, RB, NARROW>()>::BYTES + (HPCD ? GROUP_RANK_TABLE_BYTES : 0) ==  \
                group_lds_bytes(GroupInst{group_key_of<K>(), RB, KPT, DBG, NARROW, HIST2, SOA, PIPE, HPCD}), "group_lds_bytes"); \
  static_assert(group_lds_bytes(GroupInst{group_key_of<K>(), RB, KPT, DBG, NARROW, HIST2, SOA, PIPE, HPCD}) + (HIST2 ? RS_MAX_RADIX * 4 : 0) <= GROUP_LDS_MAX, \
                "the tile, the rank table and the other digit's counters fit the LDS");
MGC_GROUP_INSTS(MGC_GROUP_ROW_OK)
#undef MGC_GROUP_ROW_OK

// an instantiation that is not in the table is an error, never a neighbouring kernel
static hipError_t launch_group_pass(const GroupInst &inst, const GroupPass &p) {
#define MGC_GROUP_ROW(K, RB, KPT, DBG, NARROW, HIST2, SOA, PIPE, HPCD, BATCH)                                                         \
  if (inst == GroupInst{group_key_of<K>(), RB, KPT, DBG, NARROW, HIST2, SOA, PIPE, HPCD, BATCH})                               \
    return group_launch_form<K, RB, KPT, DBG, NARROW, HIST2, SOA, PIPE, HPCD, BATCH>(p);
  MGC_GROUP_INSTS(MGC_GROUP_ROW)
#undef MGC_GROUP_ROW
  return hipErrorInvalidValue;
}

// What the two-pass forms share once the first pass is launched (p: the second pass): the second digit's bases and the region table
// -- high digit first (msd): one kernel, off the histogram the first pass took; low digit first: the regions alone, and the shared
// look-back rows cleared again -- then the second pass and the sub-bucket boundaries off its look-back granules.
static hipError_t group_second_pass(const GroupInst &inst, const GroupPass &p, SortHeader *hdr, bool msd, u32 bits_first, u32 bits_second,
                                    uint64_t *d_sub_starts, hipEvent_t *pass_events) {
  if (pass_events) MGC_CHECK(hipEventRecord(pass_events[1], p.st));
  if (msd) {
    hipLaunchKernelGGL(narrow_mid_kernel, dim3(1), dim3(RS_MAX_RADIX), 0, p.st, hdr, p.n, (u32)group_tile(inst), p.region_start, p.region_tiles);
    MGC_CHECK(hipGetLastError());
  } else {
    hipLaunchKernelGGL(group_regions_kernel, dim3(1), dim3(RS_MAX_RADIX), 0, p.st, &hdr->gbase[0][0], p.n, (u32)group_tile(inst), p.region_start, p.region_tiles);
    MGC_CHECK(hipGetLastError());
    MGC_CHECK(hipMemsetAsync(p.status, 0, (size_t)p.tile_bound * (RS_MAX_RADIX / 2) * sizeof(u64), p.st));
  }
  if (pass_events) MGC_CHECK(hipEventRecord(pass_events[2], p.st));
  MGC_CHECK(launch_group_pass(inst, p));
  if (pass_events) MGC_CHECK(hipEventRecord(pass_events[3], p.st));
  const u64 ng = (u64)1 << (bits_first + bits_second);
  hipLaunchKernelGGL(narrow_bounds_kernel, dim3((uint32_t)((ng + 1 + 255) / 256)), dim3(256), 0, p.st, p.status, p.region_tiles,
                     p.gbase, p.n, bits_first, ng, reinterpret_cast<u64 *>(d_sub_starts), group_granules(inst));
  return hipGetLastError();
}

// mgc_device.h, GroupFile.  Low digit first: one read of the keys for both digit histograms, scratch = f.ws, physical order = key
// order.  High digit first: the histogram of the HIGH digit comes with the prepared header, the low digit's is taken by the first
// pass itself -- nobody reads the keys for a histogram -- and the physical order is (low digit : high digit).
hipError_t launch_group_narrow(GroupFile &f) {
  static_assert(MGC_NARROW_KPT0 == GROUP_KPT_NARROW0P, "mgc_group_route.hpp");
  static_assert((uint64_t)GROUP_BLOCK * GROUP_KPT_NARROW0 == NARROW_TILE0 && (uint64_t)GROUP_BLOCK * GROUP_KPT_NARROW0P == NARROW_TILE0P &&
                (uint64_t)GROUP_BLOCK * GROUP_KPT_NARROW1 == NARROW_TILE1, "narrow_scratch_bytes");
  const bool soa = f.layout == GroupKeys::SOA5, msd = f.prepared != nullptr && f.scratch != nullptr;
  bool dbg = f.dbg && msd;
  GroupInst i0, i1;
  if ((f.layout != GroupKeys::U64 && !soa) || soa != (f.soa_hi_mask != 0) || !f.plan || !sort_plan_narrows(*f.plan, f.n, 1) ||
      f.ws_bytes < sort_workspace_bytes(f.n))
    return hipErrorInvalidValue;
  const SortPlan &plan = *f.plan;
  const uint64_t n = f.n;
  const u32 low = plan.pass_shift[0], b_lo = plan.pass_bits[0], b_hi = plan.pass_bits[1];
  // first pass: digit A at shA (bA bits), dropped from the keys; second pass: digit B -- after the drop it sits at `low`
  const u32 bA = msd ? b_hi : b_lo, bB = msd ? b_lo : b_hi, shA = msd ? low + b_lo : low;
  if (!group_pick_narrow(msd, soa, f.pipe, dbg, bA, bB, &i0, &i1)) return hipErrorInvalidValue;   // the 5-byte layout: high digit first
  // f.dbg: per-phase cycle sums of the first 64 workgroups of both passes, printed (developer instrumentation; the instrumented
  // instantiations run instead of the plain ones)
  static u64 *dbg_buf = nullptr;
  if (dbg && !dbg_buf && hipMalloc(&dbg_buf, 2 * 64 * 8 * sizeof(u64)) != hipSuccess) {
    dbg_buf = nullptr; dbg = false;
    group_pick_narrow(msd, soa, f.pipe, false, bA, bB, &i0, &i1);
  }
  const uint64_t tile0 = group_tile(i0), tile1 = group_tile(i1);    // (28 words per thread in the second pass -- the most the register file takes -- measured equal: r06_ab_runs.txt)
  const uint64_t tiles0 = (n + tile0 - 1) / tile0, tiles1_max = (n + tile1 - 1) / tile1 + RS_MAX_RADIX + 1;
  constexpr size_t ROW = RS_MAX_RADIX / 2;                           // granules of a status row, whatever the instantiation uses of it
  SortHeader *hdr;
  u64 *status_a, *status_b, *region_start;
  if (msd) {
    hdr = reinterpret_cast<SortHeader *>(f.prepared);
    status_a = reinterpret_cast<u64 *>(f.scratch);
    status_b = status_a + (size_t)tiles0 * ROW;
    region_start = status_b + (size_t)tiles1_max * ROW;
  } else {
    hdr = reinterpret_cast<SortHeader *>(f.ws);
    unsigned char *body = reinterpret_cast<unsigned char *>(f.ws) + ((sizeof(SortHeader) + 255) / 256) * 256;
    status_a = status_b = reinterpret_cast<u64 *>(body);
    const size_t status_bytes = (size_t)std::max(tiles0, tiles1_max) * ROW * sizeof(u64);
    region_start = reinterpret_cast<u64 *>(body + ((status_bytes + 255) / 256) * 256);
  }
  u32 *region_tiles = reinterpret_cast<u32 *>(region_start + RS_MAX_RADIX + 1);
  f.tr_a = msd ? bA : 0u; f.tr_b = bB;

  GroupExtra ex_first{bA, 0u, 0u, nullptr};
  if (msd) ex_first = GroupExtra{bA, low, (1u << bB) - 1u, &hdr->ghist[1][0], f.soa_hi_mask};
  if (f.stagger > 1u && soa && f.pipe) { ex_first.stagger_groups = f.stagger; ex_first.stagger_cycles = NARROW_TILE0_CYCLES / f.stagger; }
  const GroupPass p0{f.keys, f.alt, (u64)n, shA, (1u << bA) - 1u, &hdr->gbase[0][0], status_a, &hdr->ticket[0], f.d_error, (u64)tiles0,
                     nullptr, nullptr, ex_first, dbg ? dbg_buf : nullptr, (u64)tiles0, f.st};
  const GroupPass p1{f.alt, f.keys, (u64)n, low, (1u << bB) - 1u, &hdr->gbase[1][0], status_b, &hdr->ticket[1], f.d_error, (u64)((n + tile1 - 1) / tile1),
                     region_start, region_tiles, GroupExtra{0u, 0u, 0u, nullptr}, dbg ? dbg_buf + 64 * 8 : nullptr, (u64)tiles1_max, f.st};
  if (!msd) {
    MGC_CHECK(group_prepare<u64>(reinterpret_cast<const u64 *>(f.keys), n, plan, hdr, f.st));   // rows 0 / 1 = low / high digit = A / B
    MGC_CHECK(hipMemsetAsync(status_a, 0, (size_t)tiles0 * ROW * sizeof(u64), f.st));
  }
  if (f.pass_events) MGC_CHECK(hipEventRecord(f.pass_events[0], f.st));
  if (dbg) MGC_CHECK(hipMemsetAsync(dbg_buf, 0, 2 * 64 * 8 * sizeof(u64), f.st));
  MGC_CHECK(launch_group_pass(i0, p0));
  MGC_CHECK(group_second_pass(i1, p1, hdr, msd, bA, bB, f.d_sub_starts, f.pass_events));
  if (dbg) {
    u64 h[2 * 64 * 8];
    MGC_CHECK(hipStreamSynchronize(f.st));
    MGC_CHECK(hipMemcpy(h, dbg_buf, sizeof(h), hipMemcpyDeviceToHost));
    for (int pass = 0; pass < 2; pass++) {
      double ps[8] = {0};
      for (int b = 0; b < 64; b++) for (int i = 0; i < 8; i++) ps[i] += (double)h[(pass * 64 + b) * 8 + i];
      const double it = ps[7] > 0 ? ps[7] : 1;
      fprintf(stderr, "[groupdbg] %s pass, %llu keys, %d-key tiles, tiles/wg=%.1f cycles/tile: ticket+zero=%.0f rank=%.0f scan+exchange=%.0f "
                      "lookback(+prefetch%s)=%.0f writeout=%.0f endsync=%.0f total=%.0f\n",
              pass ? "second (u32 -> u32)" : (soa ? (f.pipe ? "first (5 B -> u32, fetch a tile ahead)" : "first (5 B -> u32)") : "first (u64 -> u32)"), (unsigned long long)n, pass ? (int)tile1 : (int)tile0, it / 64,
              ps[0] / it, ps[1] / it, ps[2] / it, pass ? "" : ", low-digit count", ps[3] / it, ps[4] / it, ps[5] / it,
              (ps[0] + ps[1] + ps[2] + ps[3] + ps[4] + ps[5]) / it);
    }
  }
  return hipSuccess;
}

// ---- the two passes of a BATCH of narrowed files: one launch per pass and helper step (mgc_device.h, GroupBatch) ----
// Both descriptor tables ([nfiles + 1] entries each: first pass, second pass) are put together here and go to the device in one
// copy; the second pass's tile numbers are filled in on the device (narrow_mid_batch_kernel).
size_t group_batch_table_bytes(uint32_t nfiles) { return 2 * ((size_t)nfiles + 1) * sizeof(GroupBatchFile); }

hipError_t launch_group_narrow_batch(GroupBatch &b) {
  if (!b.files || !b.nfiles || !b.d_table || !b.h_table || !b.d_ctl || !b.files[0].plan) return hipErrorInvalidValue;
  const SortPlan &plan = *b.files[0].plan;
  const u32 low = plan.pass_shift[0], bB = plan.pass_bits[0], bA = plan.pass_bits[1], shA = low + bB;   // high digit (A) first
  const u32 hi_mask = b.files[0].soa_hi_mask;
  GroupInst i0, i1;
  if (!group_pick_narrow_batch(bA, bB, &i0, &i1)) return hipErrorInvalidValue;
  const uint64_t tile0 = group_tile(i0), tile1 = group_tile(i1);
  constexpr size_t ROW = RS_MAX_RADIX / 2;
  const size_t bytes = group_batch_table_bytes(b.nfiles);
  GroupBatchFile *h1 = reinterpret_cast<GroupBatchFile *>(b.h_table), *h2 = h1 + b.nfiles + 1;
  const GroupBatchFile *d1 = reinterpret_cast<const GroupBatchFile *>(b.d_table);
  GroupBatchFile *d2 = reinterpret_cast<GroupBatchFile *>(b.d_table) + b.nfiles + 1;
  memset(h1, 0, bytes);
  uint64_t at = 0, bound1 = 0;
  for (uint32_t i = 0; i < b.nfiles; i++) {
    GroupFile &f = b.files[i];
    if (f.layout != GroupKeys::SOA5 || !hi_mask || f.soa_hi_mask != hi_mask || !f.prepared || !f.scratch || !f.keys || !f.alt || !f.d_sub_starts ||
        !group_batch_form(true, true, f.pipe, f.dbg, f.stagger) || !f.plan || !sort_plan_narrows(*f.plan, f.n, 1) ||
        f.plan->pass_shift[0] != low || f.plan->pass_bits[0] != bB || f.plan->pass_bits[1] != bA)
      return hipErrorInvalidValue;
    const uint64_t tiles0 = (f.n + tile0 - 1) / tile0, tiles1_max = (f.n + tile1 - 1) / tile1 + RS_MAX_RADIX + 1;
    SortHeader *hdr = reinterpret_cast<SortHeader *>(f.prepared);          // (the scratch is laid out as launch_group_narrow lays it out)
    u64 *status_a = reinterpret_cast<u64 *>(f.scratch), *status_b = status_a + (size_t)tiles0 * ROW;
    u64 *region_start = status_b + (size_t)tiles1_max * ROW;
    u32 *region_tiles = reinterpret_cast<u32 *>(region_start + RS_MAX_RADIX + 1);
    h1[i] = GroupBatchFile{(u64)at, (u64)tiles0, (u64)f.n, f.keys, f.alt, &hdr->gbase[0][0], status_a, &hdr->ghist[1][0], nullptr, nullptr, nullptr};
    h2[i] = GroupBatchFile{0, 0, (u64)f.n, f.alt, f.keys, &hdr->gbase[1][0], status_b, nullptr, region_start, region_tiles,
                           reinterpret_cast<u64 *>(f.d_sub_starts)};
    at += tiles0; bound1 += tiles1_max;
    f.tr_a = bA; f.tr_b = bB;
  }
  h1[b.nfiles].tile0 = at;
  if (bound1 >= (1ull << 32)) return hipErrorInvalidValue;                 // tickets are 32-bit words
  MGC_CHECK(hipMemcpyAsync(b.d_table, b.h_table, bytes, hipMemcpyHostToDevice, b.st));
  if (b.pass_events) MGC_CHECK(hipEventRecord(b.pass_events[0], b.st));
  GroupPass p0{nullptr, nullptr, 0, shA, (1u << bA) - 1u, nullptr, nullptr, b.d_ctl, b.d_error, (u64)at, nullptr, nullptr,
               GroupExtra{bA, low, (1u << bB) - 1u, nullptr, hi_mask}, nullptr, (u64)at, b.st};
  p0.bfiles = d1; p0.nbf = b.nfiles;
  MGC_CHECK(launch_group_pass(i0, p0));
  if (b.pass_events) MGC_CHECK(hipEventRecord(b.pass_events[1], b.st));
  hipLaunchKernelGGL(narrow_mid_batch_kernel, dim3(b.nfiles), dim3(RS_MAX_RADIX), 0, b.st, d1, d2, (u32)b.nfiles, (u32)tile1, b.d_ctl + 2);
  MGC_CHECK(hipGetLastError());
  if (b.pass_events) MGC_CHECK(hipEventRecord(b.pass_events[2], b.st));
  GroupPass p1{nullptr, nullptr, 0, low, (1u << bB) - 1u, nullptr, nullptr, b.d_ctl + 1, b.d_error, 0, nullptr, nullptr,
               GroupExtra{0u, 0u, 0u, nullptr}, nullptr, (u64)bound1, b.st};
  p1.bfiles = d2; p1.nbf = b.nfiles;
  MGC_CHECK(launch_group_pass(i1, p1));
  if (b.pass_events) MGC_CHECK(hipEventRecord(b.pass_events[3], b.st));
  const u64 ng = (u64)1 << (bA + bB);
  hipLaunchKernelGGL(narrow_bounds_batch_kernel, dim3((uint32_t)((ng + 1 + 255) / 256), b.nfiles), dim3(256), 0, b.st,
                     (const GroupBatchFile *)d2, bA, ng, group_granules(i1));
  return hipGetLastError();
}

// ---- the same two passes for WHOLE keys (mgc_device.h, launch_group_wide) ----
bool sort_plan_wide_msd(const SortPlan &plan, uint64_t n, bool on) {
  return on && plan.mode == 3 && plan.num_passes == 2 && plan.radix_bits == 9 && n > 0 && n < (1ull << 30) &&
         plan.pass_shift[1] == plan.pass_shift[0] + plan.pass_bits[0];
}

// one workgroup per bucket: header cleared, histogram of the bucket's high dense-rank digit from the dense-rank table, its scan
struct HpcPrep { u32 bucket_bits; u64 on[4]; };
__global__ __launch_bounds__(RS_MAX_RADIX)
void hpc_prepare_kernel(const u64 *__restrict__ fine, HpcPrep prep, unsigned char *__restrict__ hdrs, u32 hdr_stride) {
  __shared__ u64 s_tmp[RS_MAX_RADIX / 64 + 1];
  const u32 b = blockIdx.x, x = threadIdx.x;
  if (!((prep.on[b >> 6] >> (b & 63u)) & 1ull)) return;
  SortHeader *hdr = reinterpret_cast<SortHeader *>(hdrs + (size_t)b * hdr_stride);
  u32 *w = reinterpret_cast<u32 *>(hdr);
  for (u32 i = x; i < sizeof(SortHeader) / 4; i += RS_MAX_RADIX) w[i] = 0;
  const u32 bb = prep.bucket_bits / 2;                       // dense rank of the bucket's bases (a bucket with k-mers repeats none)
  u32 prev = (b >> (2 * bb - 2)) & 3u, r = prev;
  for (u32 i = 1; i < bb; i++) { const u32 c = (b >> (2 * (bb - 1 - i))) & 3u; r = r * 3u + (c - (c > prev ? 1u : 0u)); prev = c; }
  const u64 c = (x < 243u) ? fine[(size_t)r * 243u + x] : 0ull;
  __syncthreads();                                           // (the header is cleared)
  u64 total;
  const u64 e = block_excl_scan<RS_MAX_RADIX, u64>(c, s_tmp, &total);
  hdr->ghist[0][x] = c;
  hdr->gbase[0][x] = e;
}

hipError_t launch_hpc_prepare(const uint64_t *d_fine_hpc, uint32_t bucket_bits, const uint64_t on[4], void *d_hdrs, hipStream_t st) {
  if (bucket_bits != 6 && bucket_bits != 8) return hipErrorInvalidValue;
  HpcPrep prep;
  prep.bucket_bits = bucket_bits;
  for (int i = 0; i < 4; i++) prep.on[i] = on[i];
  hipLaunchKernelGGL(hpc_prepare_kernel, dim3(1u << bucket_bits), dim3(RS_MAX_RADIX), 0, st, reinterpret_cast<const u64 *>(d_fine_hpc), prep,
                     reinterpret_cast<unsigned char *>(d_hdrs), (u32)sort_header_bytes());
  return hipGetLastError();
}

// (the look-back scratch is sized for the SMALLEST tile of any whole-key instantiation of a key width: K128 8192 keys, K96 12288 --
// launch_group_wide asserts that its tiles are not smaller)
static inline uint64_t wide_tile(uint32_t key_words) { return key_words == 2 ? 1024u * 8u : 1024u * 16u; }
size_t wide_scratch_bytes(uint64_t n, uint32_t key_words) {
  const uint64_t tile = wide_tile(key_words);
  const uint64_t tiles0 = (n + tile - 1) / tile, tiles1_max = tiles0 + RS_MAX_RADIX + 1;
  return (size_t)(tiles0 + tiles1_max) * (RS_MAX_RADIX / 2) * sizeof(u64) + (size_t)(RS_MAX_RADIX + 2) * 16 + 512;
}

hipError_t launch_group_wide(GroupFile &f) {
  static_assert((uint64_t)GROUP_BLOCK * group_kpt_wide(GROUP_U64) >= 1024u * 16u && (uint64_t)GROUP_BLOCK * group_kpt_wide(GROUP_K128) >= 1024u * 8u &&
                (uint64_t)GROUP_BLOCK * group_kpt_wide(GROUP_K96) >= 1024u * 8u, "wide_scratch_bytes sizes the granules for tiles of at least wide_tile() keys");
  if (!f.plan || !sort_plan_wide_msd(*f.plan, f.n) || !f.prepared || !f.scratch ||
      (f.layout != GroupKeys::U64 && f.layout != GroupKeys::K128 && f.layout != GroupKeys::K96))
    return hipErrorInvalidValue;
  const SortPlan &plan = *f.plan;
  const uint64_t n = f.n;
  // the keys stay whole: digit A (high) at shA, digit B (low) at `low`, both where the plan put them
  // (`compress`: dense-rank digits in ten-bit fields -- the kernels take the digit with hpc_digit(), the sub-bucket numbers keep the fields)
  const u32 low = plan.pass_shift[0], bB = plan.pass_bits[0], bA = plan.pass_bits[1], shA = low + bB;
  const u32 maskA = plan_mask(plan, 1), maskB = plan_mask(plan, 0);
  GroupInst i0, i1;
  group_pick_wide(f.layout == GroupKeys::U64 ? GROUP_U64 : (f.layout == GroupKeys::K128 ? GROUP_K128 : GROUP_K96), plan.hpc, bB, bA, &i0, &i1);
  const uint64_t tile = group_tile(i0);                      // (both passes: 12-byte K96 records take 12288-key tiles, 144 KiB of LDS)
  const uint64_t tiles0 = (n + tile - 1) / tile, tiles1_max = tiles0 + RS_MAX_RADIX + 1;
  const size_t row = group_granules(i0);                     // granules of a status row
  SortHeader *hdr = reinterpret_cast<SortHeader *>(f.prepared);
  u64 *status_a = reinterpret_cast<u64 *>(f.scratch);
  u64 *status_b = status_a + (size_t)tiles0 * row;
  u64 *region_start = status_b + (size_t)tiles1_max * row;
  u32 *region_tiles = reinterpret_cast<u32 *>(region_start + RS_MAX_RADIX + 1);
  f.tr_a = bA; f.tr_b = bB;

  const GroupPass p0{f.keys, f.alt, (u64)n, shA, maskA, &hdr->gbase[0][0], status_a, &hdr->ticket[0], f.d_error, (u64)tiles0,
                     nullptr, nullptr, GroupExtra{0u, low, maskB, &hdr->ghist[1][0]}, nullptr, (u64)tiles0, f.st};
  const GroupPass p1{f.alt, f.keys, (u64)n, low, maskB, &hdr->gbase[1][0], status_b, &hdr->ticket[1], f.d_error, (u64)tiles0,
                     region_start, region_tiles, GroupExtra{0u, 0u, 0u, nullptr}, nullptr, (u64)tiles1_max, f.st};
  if (f.pass_events) MGC_CHECK(hipEventRecord(f.pass_events[0], f.st));
  MGC_CHECK(launch_group_pass(i0, p0));
  return group_second_pass(i1, p1, hdr, true, bA, bB, f.d_sub_starts, f.pass_events);
}

size_t sort_header_bytes() { return ((sizeof(SortHeader) + 255) / 256) * 256; }

hipError_t launch_radix_sort(void *d_keys, void *d_alt, uint64_t n, uint32_t key_words, const SortPlan &plan,
                             void *d_ws, size_t ws_bytes, uint32_t *d_error, int *result_in_alt,
                             hipStream_t st, hipEvent_t *pass_events) {
  *result_in_alt = 0;
  if (n == 0 || plan.num_passes == 0) return hipSuccess;
  if (ws_bytes < sort_workspace_bytes(n)) return hipErrorInvalidValue;
  if (plan.hpc && !(plan.mode == 3 && plan.num_passes <= 2 && n < (1ull << 30))) return hipErrorInvalidValue;
  if (plan.mode == 3 && (plan.num_passes > 2 || n >= (1ull << 30))) {
    SortPlan stable = plan;                 // grouping is defined for one or two digits and 30-bit granule values
    stable.mode = 0;
    return launch_radix_sort(d_keys, d_alt, n, key_words, stable, d_ws, ws_bytes, d_error, result_in_alt, st, pass_events);
  }
  // packed look-back granules hold 30-bit values: larger calls use the wide ones; 16-byte keys: 8 per thread keep the tile at 128 KiB
  if (key_words == 2) {
    if (n >= (1ull << 30)) return run_passes<K128, 8, 3>(d_keys, d_alt, n, plan, d_ws, d_error, result_in_alt, st, pass_events);
    return run_passes<K128, 8, 2>(d_keys, d_alt, n, plan, d_ws, d_error, result_in_alt, st, pass_events);
  }
  if (n >= (1ull << 30)) return run_passes<u64, 16, 3>(d_keys, d_alt, n, plan, d_ws, d_error, result_in_alt, st, pass_events);
  return run_passes<u64, 16, 2>(d_keys, d_alt, n, plan, d_ws, d_error, result_in_alt, st, pass_events);
}



hipError_t warm_sort() { hipFuncAttributes a; return hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&narrow_mid_kernel)); }

}  // namespace mgc
