// gzip_host.cpp -- meryl_amd/csrc/mgc_gzip_par.hpp stand-alone: one gzip file through gz_run, the markers resolved here on the
// CPU (what mgc_gzip.hip does on the device), every member's CRC32 and ISIZE compared with its trailer.  Prints one line of
// key=value fields.  Built plain and with sanitizers by tests/test_gzip_host.py.
//
//   gzip_host FILE SPAN CAP THREADS [FORCE_SPAN FORCE_BIT [DELAY_SPAN0_MS]]     (FORCE_SPAN -1: none)
#include "../../meryl_amd/csrc/mgc_gzip_par.hpp"

#include <cstdio>
#include <cstdlib>
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

int main(int argc, char **argv) {
  if (argc < 5) { fprintf(stderr, "usage: gzip_host FILE SPAN CAP THREADS [FORCE_SPAN FORCE_BIT]\n"); return 2; }
  const int fd = open(argv[1], O_RDONLY);
  struct stat st;
  if (fd < 0 || fstat(fd, &st) != 0) { perror(argv[1]); return 2; }
  const uint64_t size = (uint64_t)st.st_size;
  const uint8_t *map = size ? static_cast<const uint8_t *>(mmap(nullptr, size, PROT_READ, MAP_SHARED, fd, 0)) : reinterpret_cast<const uint8_t *>("");
  if (map == MAP_FAILED) { perror("mmap"); return 2; }
  mgc::GzOptions opt;
  opt.span = strtoull(argv[2], nullptr, 10);
  opt.cap = strtoull(argv[3], nullptr, 10);
  opt.threads = atoi(argv[4]);
  opt.n_slots = opt.threads + 4;
  if (argc >= 7 && argv[5][0] != '-') { opt.force_span = strtoull(argv[5], nullptr, 10); opt.force_bit = strtoull(argv[6], nullptr, 10); }
  if (argc >= 8) opt.delay_span0_ms = atoi(argv[7]);

  std::vector<char *> slots((size_t)std::max(opt.n_slots, opt.lag + 3), nullptr);
  std::vector<uint8_t> window(mgc::GZ_WINDOW, 0), text;
  uint64_t total = 0, max_piece = 0, min_window = mgc::GZ_WINDOW;        // min_window: over the pieces that hold markers
  uint32_t crc_all = 0, crc_member = 0;
  uint64_t member_len = 0;
  const char *bad = nullptr;
  uint64_t bad_off = 0;
  auto consume = [&](const mgc::GzPieceView &v) -> int {
    text.assign(v.text, v.text + v.text_len);
    if (v.n_symbols > v.text_len) { bad = "prefix"; return 1; }
    if (v.n_symbols) min_window = std::min<uint64_t>(min_window, v.window_valid);
    for (uint64_t i = 0; i < v.n_symbols; i++) {
      const uint16_t s = v.symbols[i];
      if (s < 256) { if (s != text[i]) { bad = "prefix_text"; return 1; } continue; }
      if (s < mgc::GZ_MARK || (uint32_t)(s - mgc::GZ_MARK) < mgc::GZ_WINDOW - v.window_valid) { bad = "marker"; bad_off = v.comp_off; return 1; }
      text[i] = window[s - mgc::GZ_MARK];
    }
    // the next window: the last 32 KiB of (window ++ text)
    if (text.size() >= mgc::GZ_WINDOW) window.assign(text.end() - mgc::GZ_WINDOW, text.end());
    else { window.erase(window.begin(), window.begin() + (long)text.size()); window.insert(window.end(), text.begin(), text.end()); }
    uint64_t from = 0;
    for (size_t e = 0; e < v.n_ends; e++) {
      const mgc::GzMemberEnd &m = v.ends[e];
      crc_member = (uint32_t)crc32(crc_member, text.data() + from, (uInt)(m.text_off - from));
      member_len += m.text_off - from;
      if (crc_member != m.crc) { bad = "crc"; bad_off = m.comp_off; return 1; }
      if ((uint32_t)member_len != m.isize) { bad = "isize"; bad_off = m.comp_off; return 1; }
      crc_member = 0; member_len = 0; from = m.text_off;
    }
    crc_member = (uint32_t)crc32(crc_member, text.data() + from, (uInt)(text.size() - from));
    member_len += text.size() - from;
    crc_all = (uint32_t)crc32(crc_all, text.data(), (uInt)text.size());
    total += text.size();
    max_piece = std::max<uint64_t>(max_piece, text.size());
    return 0;
  };
  const mgc::GzResult r = mgc::gz_run(map, size, opt, slots.data(), [&]() { return static_cast<char *>(malloc(opt.cap)); }, consume);
  for (char *p : slots) free(p);
  if (r.end == mgc::GzResult::FORMAT) printf("status=format err=%d off=%llu\n", r.detail, (unsigned long long)r.offset);
  else if (r.end == mgc::GzResult::CONSUMER_STOPPED) printf("status=%s off=%llu\n", bad ? bad : "stopped", (unsigned long long)bad_off);
  else if (r.end != mgc::GzResult::DONE) printf("status=alloc\n");
  else
    printf("status=ok len=%llu crc=%u members=%llu chunks=%llu confirmed=%llu discarded=%llu cuts=%llu symbol_bytes=%llu max_piece=%llu min_window=%llu\n",
           (unsigned long long)total, crc_all, (unsigned long long)r.info.members, (unsigned long long)r.info.chunks, (unsigned long long)r.info.confirmed,
           (unsigned long long)r.info.discarded, (unsigned long long)r.info.cuts, (unsigned long long)r.info.symbol_bytes, (unsigned long long)max_piece, (unsigned long long)min_window);
  return 0;
}
