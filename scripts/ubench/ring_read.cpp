// Reader-ring microbenchmark: the read side of mgc_push_text_file without the device (does the ring let N readers run in
// parallel on this box, into malloc'ed and into hipHostMalloc'ed buffers?).  The ring is the one that ships (mgc_chunk_ring.hpp).
// hipcc ring_read.cpp -o ring_read -lpthread        ring_read FILE READERS PINNED(0|1) [SLOTS]
#include "../../meryl_amd/csrc/mgc_chunk_ring.hpp"
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>
int main(int argc, char **argv) {
  const char *path = argv[1]; int reader_threads = atoi(argv[2]); const bool pinned = atoi(argv[3]) != 0; const int R = argc > 4 ? atoi(argv[4]) : 8;
  int fd = open(path, O_RDONLY); struct stat st; fstat(fd, &st); uint64_t size = st.st_size;
  const size_t CH = 32u << 20; const uint64_t nchunks = (size + CH - 1) / CH;
  std::vector<char *> ring(R);
  for (int i = 0; i < R; i++) {
    if (pinned) { if (hipHostMalloc((void **)&ring[i], CH, hipHostMallocDefault) != hipSuccess) { printf("hipHostMalloc failed\n"); return 1; } }
    else ring[i] = (char *)malloc(CH);
    memset(ring[i], 1, CH);
  }
  auto fill = [&](int, uint64_t c, char *dst, int *) -> int64_t {
    const uint64_t off = c * CH; const size_t want = (size_t)std::min<uint64_t>(CH, size - off); size_t have = 0;
    while (have < want) { ssize_t r = pread(fd, dst + have, want - have, off + have); if (r <= 0) break; have += r; }
    return (int64_t)have; };
  const double t0 = mgc::now_s();
  const mgc::ChunkRingResult res = mgc::run_chunk_ring(nchunks, ring.data(), R, reader_threads, 2, []() -> char * { return nullptr; }, fill,
                                                       [](uint64_t, const char *, size_t) { return 0; });
  const double dt = mgc::now_s() - t0;
  printf("%2d readers, ring %2d, %s: %.2f GB in %.3f s = %5.1f GB/s; per-thread pread rate %.1f GB/s\n", reader_threads, R, pinned ? "pinned" : "malloc",
         size / 1e9, dt, size / 1e9 / dt, size / 1e9 / res.t_fill);
}
