// mgc_textfile.cpp -- whole FASTA / FASTQ / SAM files into a session's base stream (include/meryl_gpu_count.h): plain files read
// with pread, BGZF files inflated, by several threads STRAIGHT into a ring of pinned buffers (mgc_chunk_ring.hpp) that the
// calling thread uploads and parses in file order; BGZF BAM files likewise, walked and decoded instead of parsed; plain gzip files
// through the pump of mgc_gzip_par.hpp, whose pieces the device resolves (mgc_gzip.hip).  The session is reached through mgc_begin_text /
// mgc_end_text / mgc_begin_bam and what mgc_session.hpp declares of mgc_input.cpp (text_submit / bam_submit / gzip_submit, text_drain,
// text_rollback, refuse_file and its BAM / gzip forms, bam_end, the ring's pinned file slots, the gzip ledger's verdict) only.
#include "../../include/meryl_gpu_count.h"
#include "mgc_bgzf.hpp"
#include "mgc_chunk_ring.hpp"
#include "mgc_gzip_par.hpp"
#include "mgc_session.hpp"

#include <algorithm>
#include <cerrno>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>
#include <vector>

using mgc::set_err;

namespace {
// `path` opened for reading if it is a regular file (a `kind`) of at least min_size bytes, or -1 and why not in *err
int open_regular(std::string *err, const char *who, const char *path, const char *kind, off_t min_size, uint64_t *size) {
  const int fd = open(path, O_RDONLY);
  if (fd < 0) { set_err(err, "%s: cannot open '%s': %s", who, path, strerror(errno)); return -1; }
  struct stat st;
  if (fstat(fd, &st) != 0 || !S_ISREG(st.st_mode) || st.st_size < min_size) { close(fd); set_err(err, "%s: '%s' is not a %s", who, path, kind); return -1; }
  *size = (uint64_t)st.st_size;
  return fd;
}

// the first byte of text that is not white space; 0: none
char first_text_byte(const unsigned char *p, size_t n) {
  for (size_t i = 0; i < n; i++) if (p[i] != '\n' && p[i] != '\r' && p[i] != ' ' && p[i] != '\t') return (char)p[i];
  return 0;
}
int format_of(char c) { return c == '@' ? MGC_TEXT_FASTQ : (c == '>' ? MGC_TEXT_FASTA : 0); }

// format of a FASTA / FASTQ file from its first byte that is not white space; 0: neither (SAM is never sniffed: its header lines
// start with '@' as FASTQ records do, so it is asked for by name)
int sniff_text_format(int fd, char *first) {
  unsigned char head[4096];
  const ssize_t got = pread(fd, head, sizeof(head), 0);
  char c = first_text_byte(head, got > 0 ? (size_t)got : 0);
  if (!c) c = '>';
  if (first) *first = c;
  return format_of(c);
}

// The ring of a session: its pinned slots are allocated by the producers themselves, in parallel, on first use, and stay
// with the session for the next file (mgc_close frees them).  lag 2: see run_chunk_ring.
inline auto slot_alloc(mgc_session *s) { return [s]() { return mgc::InputRing::alloc_file_slot(s->device, mgc_session::TEXT_CHUNK); }; }
template <class Fill, class Consume>
mgc::ChunkRingResult run_session_ring(mgc_session *s, uint64_t n_chunks, const mgc::ChunkRingGeometry &g, Fill fill, Consume consume) {
  return mgc::run_chunk_ring(n_chunks, s->in.file_slots, g.slots, g.threads, 2, slot_alloc(s), fill, consume);
}
bool known_format(int format) { return format == MGC_TEXT_FASTA || format == MGC_TEXT_FASTQ || format == MGC_TEXT_SAM; }
}  // namespace

// First record start at or after `offset` of a FASTA / FASTQ file -- where a reader that takes the file from the middle
// may begin (the ranks of a node count read disjoint byte windows of the input, each through its own device's link).
// FASTA: a line that starts with '>'.  FASTQ (four-line records): a line that starts with '@' whose next-but-one line starts
// with '+' -- a quality line may start with '@', but then the line two below it is a sequence line, never '+'.  SAM: any line start.
extern "C" int mgc_text_record_start(const char *path, int format, uint64_t offset, uint64_t *start) {
  if (!path || !start) return MGC_EINVAL;
  uint64_t size = 0;
  const int fd = open_regular(nullptr, "mgc_text_record_start", path, "regular file", 0, &size);
  if (fd < 0) return MGC_EINVAL;
  if (format == 0) format = sniff_text_format(fd, nullptr);
  if (!known_format(format)) { close(fd); set_err(nullptr, "'%s' is neither FASTA nor FASTQ", path); return MGC_EFORMAT; }
  if (offset == 0 || offset >= size) { close(fd); *start = offset >= size ? size : 0; return MGC_OK; }
  // line starts from offset - 1 on: the byte before a line start is '\n'
  std::vector<char> buf(1u << 20);
  uint64_t pos = offset - 1;                               // file position of buf[0]
  std::vector<uint64_t> ls;                                // line starts found so far (file offsets), with their first byte
  std::vector<char> lc;
  uint64_t answer = size;
  bool found = false;
  while (!found && pos < size) {
    const ssize_t got = pread(fd, buf.data(), buf.size(), (off_t)pos);
    if (got <= 0) break;
    for (ssize_t i = 0; i < got && !found; i++) {
      if (buf[i] != '\n') continue;
      const uint64_t line = pos + (uint64_t)i + 1;
      if (line >= size) break;
      char c;
      if (i + 1 < got) c = buf[i + 1];
      else if (pread(fd, &c, 1, (off_t)line) != 1) break;
      if (format == MGC_TEXT_SAM) { answer = line; found = true; continue; }
      if (format == MGC_TEXT_FASTA) { if (c == '>') { answer = line; found = true; } continue; }
      ls.push_back(line); lc.push_back(c);
      const size_t m = ls.size();
      if (m >= 3 && lc[m - 3] == '@' && lc[m - 1] == '+') { answer = ls[m - 3]; found = true; }
    }
    pos += (uint64_t)got;
  }
  close(fd);
  *start = found ? answer : size;
  return MGC_OK;
}

// A whole uncompressed FASTA/FASTQ file: `reader_threads` threads pread() 32 MiB chunks straight into the ring of pinned
// buffers (no intermediate copy), the calling thread uploads and parses them in file order.  A 20 GB FASTQ on tmpfs is
// otherwise bound by ONE thread's read()+memcpy (measured 11 GB/s, 1.8 s of a 3 s file -> database run).
extern "C" int mgc_push_text_file(mgc_session *s, const char *path, int format, int reader_threads) {
  return mgc_push_text_file_range(s, path, format, reader_threads, 0, ~0ull);
}

// bytes [range_begin, range_end) of the file (range_begin at a record start; range_end = the next reader's start, or past the end)
extern "C" int mgc_push_text_file_range(mgc_session *s, const char *path, int format, int reader_threads, uint64_t range_begin, uint64_t range_end) {
  if (!s || !path) return MGC_EINVAL;
  uint64_t file_size = 0;
  const int fd = open_regular(&s->err, "mgc_push_text_file", path, "regular file", 0, &file_size);
  if (fd < 0) return MGC_EINVAL;
  if (format == 0) {
    char c = 0;
    format = sniff_text_format(fd, &c);
    if (!format) { close(fd); set_err(&s->err, "'%s' is neither FASTA nor FASTQ (record starts with '%c')", path, c); return MGC_EFORMAT; }
  }
  if (!known_format(format)) { close(fd); return MGC_EINVAL; }
  if (range_end > file_size) range_end = file_size;
  if (range_begin > range_end) range_begin = range_end;
  const uint64_t size = range_end - range_begin;            // every chunk offset below is relative to the window
  int rc = mgc_begin_text(s, format);
  if (rc != MGC_OK) { close(fd); return rc; }

  const size_t CH = mgc_session::TEXT_CHUNK;
  const uint64_t nchunks = (size + CH - 1) / CH;
  const mgc::ChunkRingGeometry g = mgc::chunk_ring_geometry(reader_threads, nchunks, mgc_session::TEXT_RING_MAX);
  auto fill = [&](int, uint64_t c, char *dst, int *err_no) -> int64_t {
    const uint64_t off = c * CH;
    const size_t want = (size_t)std::min<uint64_t>(CH, size - off);
    size_t have = 0;
    while (have < want) {
      const ssize_t r = pread(fd, dst + have, want - have, (off_t)(range_begin + off + have));
      if (r < 0 && errno == EINTR) continue;
      if (r <= 0) { *err_no = r < 0 ? errno : 0; return -1; }          // an error, or the file shrank under us
      have += (size_t)r;
    }
    return (int64_t)have;
  };
  const mgc::ChunkRingResult res = run_session_ring(s, nchunks, g, fill, [&](uint64_t, const char *p, size_t len) { return mgc::text_submit(s, p, len); });
  mgc::text_drain(s);                                       // the last uploads still read from the ring
  close(fd);
  if (res.end == mgc::ChunkRingResult::ALLOC_FAILED) { set_err(&s->err, "mgc_push_text_file: pinned buffers: out of memory"); (void)mgc_end_text(s); return MGC_ENOMEM; }
  if (getenv("MGC_IO_TRACE"))
    fprintf(stderr, "[io] %s file %.2f GB in %llu chunks, %d readers, ring %d: waiting for readers %.3f s, upload+parse submit (incl. waits "
                    "for the device) %.3f s; readers: %.3f s in pread (%.1f GB/s each), %.3f s waiting for a free slot\n",
            format == MGC_TEXT_SAM ? "SAM" : "text", size / 1e9, (unsigned long long)nchunks, g.threads, g.slots, res.t_wait, res.t_consume, res.t_fill,
            res.t_fill > 0 ? size / 1e9 / res.t_fill : 0.0, res.t_slot_wait);
  if (res.end == mgc::ChunkRingResult::CONSUMER_STOPPED) rc = res.detail;
  if (res.end == mgc::ChunkRingResult::FILL_FAILED) {
    set_err(&s->err, "mgc_push_text_file: reading '%s' failed: %s", path, res.detail ? strerror(res.detail) : "the file shrank");
    rc = MGC_EINVAL;
  }
  const int rc_end = mgc_end_text(s);                       // closes the file in every case (rolls it back on MGC_EFORMAT)
  return rc != MGC_OK ? rc : rc_end;
}

// ---- a BGZF file (bgzip'd FASTA / FASTQ; mgc_bgzf.hpp) inflated by `threads` threads STRAIGHT into the pinned upload ring (round 6) ----
// Through the generic reader (meryl_seq.cpp: BgzfSource -> msr_read_text -> mgc_push_text) the text of a batch of blocks was copied twice
// by the calling thread (out of the inflater's batch, into the pinned buffer) behind batches of 32 MiB whose threads were spawned per
// batch: 4 GB/s of text with 32 threads (profiles/r06w: bench.py e2e_compressed).  Here the file is mapped, its blocks are indexed in one
// walk over the headers, chunks of <= TEXT_CHUNK of text are handed to persistent worker threads that inflate block after block into the
// chunk's ring slot, and the calling thread uploads and parses the chunks in order.
extern "C" int mgc_is_bgzf_file(const char *path) {
  if (!path) return 0;
  const int fd = open(path, O_RDONLY);
  if (fd < 0) return 0;
  unsigned char head[64];
  const ssize_t got = pread(fd, head, sizeof(head), 0);
  close(fd);
  mgc::BgzfBlock b;
  return (got >= 18 && mgc::bgzf_parse_block(head, (size_t)got, &b) != mgc::BGZF_NOT_BLOCK) ? 1 : 0;
}

namespace {
// A BGZF file for the chunk ring: mapped, its blocks planned into chunks of <= TEXT_CHUNK of text, one inflater per worker thread.
struct BgzfFile {
  int fd = -1;
  const unsigned char *map = nullptr;
  uint64_t fsize = 0;
  mgc::BgzfPlan plan;
  mgc::ChunkRingGeometry g;
  std::vector<z_stream> zs;                                     // one inflater per worker thread, n_z of them set up
  int n_z = 0;

  // MGC_OK, or the code to return with the session's error set (`who`: the calling function's name)
  int open(mgc_session *s, const char *who, const char *path, int threads) {
    fd = open_regular(&s->err, who, path, "regular BGZF file", 28, &fsize);
    if (fd < 0) return MGC_EINVAL;
    void *m = mmap(nullptr, fsize, PROT_READ, MAP_SHARED, fd, 0);
    if (m == MAP_FAILED) { set_err(&s->err, "%s: mmap of '%s' failed: %s", who, path, strerror(errno)); return MGC_EINVAL; }
    map = static_cast<const unsigned char *>(m);
    plan = mgc::bgzf_plan_chunks(map, fsize, mgc_session::TEXT_CHUNK);
    if (plan.bad != mgc::BGZF_BLOCK) {
      if (plan.bad == mgc::BGZF_BAD_ISIZE) set_err(&s->err, "'%s': corrupt BGZF block at offset %zu (ISIZE %u)", path, (size_t)plan.bad_off, plan.bad_isize);
      else set_err(&s->err, "'%s': not a BGZF block at offset %zu (plain gzip data, or a truncated file)", path, (size_t)plan.bad_off);
      return MGC_EFORMAT;
    }
    g = mgc::chunk_ring_geometry(threads, plan.chunks.size(), mgc_session::TEXT_RING_MAX);
    zs.resize(g.threads);
    while (n_z < g.threads && inflateInit2(&zs[n_z], -15) == Z_OK) n_z++;
    if (n_z < g.threads) { set_err(&s->err, "zlib: inflateInit2 failed"); return MGC_ENOMEM; }
    return MGC_OK;
  }
  bool inflate_block(int t, size_t i, unsigned char *dst) { return mgc::bgzf_inflate_block(zs[t], map + plan.blocks[i].off, plan.blocks[i], dst); }
  // the ring's fill: worker t inflates the blocks of chunk c into dst; -1 and the block's number when one does not inflate
  int64_t fill(int t, uint64_t c, char *dst, int *bad_block) {
    size_t at = 0;
    for (size_t i = plan.chunks[c].first; i < plan.chunks[c].last; i++) {
      if (!inflate_block(t, i, reinterpret_cast<unsigned char *>(dst) + at)) { *bad_block = (int)i; return -1; }
      at += plan.blocks[i].isize;
    }
    return (int64_t)at;
  }
  // A block did not inflate: what the file has put into the stream is taken back (as for a file that stops being strict FASTQ), unless
  // part of it already went into a counted batch
  static int refuse_block(mgc_session *s, const char *path, int block) {
    char why[80];
    snprintf(why, sizeof(why), "BGZF block %llu failed to inflate", (unsigned long long)block);
    return mgc::refuse_file(s, path, why, " ", " (corrupt file)");
  }
  BgzfFile() = default;
  BgzfFile(const BgzfFile &) = delete;
  BgzfFile &operator=(const BgzfFile &) = delete;
  ~BgzfFile() {
    for (int t = 0; t < n_z; t++) inflateEnd(&zs[t]);
    if (map) munmap(const_cast<unsigned char *>(map), fsize);
    if (fd >= 0) close(fd);
  }
};
}  // namespace

extern "C" int mgc_push_text_bgzf_file(mgc_session *s, const char *path, int format, int threads) {
  if (!s || !path) return MGC_EINVAL;
  BgzfFile f;
  int rc = f.open(s, "mgc_push_text_bgzf_file", path, threads);
  if (rc != MGC_OK) return rc;
  const std::vector<mgc::BgzfBlock> &blocks = f.plan.blocks;
  if (format == 0) {                                            // sniff: the first byte of text that is not white space
    char c = 0;
    std::vector<unsigned char> tmp(65536);
    for (size_t i = 0; i < blocks.size() && !c; i++) {
      if (!f.inflate_block(0, i, tmp.data())) { set_err(&s->err, "'%s': BGZF block %zu failed to inflate (corrupt file)", path, i); return MGC_EFORMAT; }
      c = first_text_byte(tmp.data(), blocks[i].isize);
    }
    format = format_of(c);
    if (!format) { set_err(&s->err, "'%s' is neither FASTA nor FASTQ (record starts with '%c')", path, c ? c : '?'); return MGC_EFORMAT; }
  }
  rc = mgc_begin_text(s, format);
  if (rc != MGC_OK) return rc;

  uint64_t text_total = 0;
  auto consume = [&](uint64_t, const char *p, size_t len) {
    text_total += len;
    return len ? mgc::text_submit(s, p, len) : MGC_OK;          // (a chunk of empty blocks: the end-of-file marker)
  };
  const uint64_t nchunks = f.plan.chunks.size();
  const mgc::ChunkRingResult res = run_session_ring(s, nchunks, f.g, [&f](int t, uint64_t c, char *dst, int *bad) { return f.fill(t, c, dst, bad); }, consume);
  mgc::text_drain(s);                                           // the last uploads still read from the ring
  if (getenv("MGC_IO_TRACE"))
    fprintf(stderr, "[io] BGZF %sfile %.2f GB -> %.2f GB of text in %llu chunks (%zu blocks), %d inflaters, ring %d: waiting for the inflaters %.3f s, "
                    "upload+parse submit (incl. waits for the device) %.3f s\n", format == MGC_TEXT_SAM ? "SAM " : "", f.fsize / 1e9, text_total / 1e9, (unsigned long long)nchunks, blocks.size(),
            f.g.threads, f.g.slots, res.t_wait, res.t_consume);
  if (res.end == mgc::ChunkRingResult::ALLOC_FAILED) { set_err(&s->err, "mgc_push_text_bgzf_file: pinned buffers: out of memory"); (void)mgc_end_text(s); return MGC_ENOMEM; }
  if (res.end == mgc::ChunkRingResult::FILL_FAILED) return BgzfFile::refuse_block(s, path, res.detail);
  if (res.end == mgc::ChunkRingResult::CONSUMER_STOPPED) rc = res.detail;
  const int rc_end = mgc_end_text(s);                           // closes the file in every case (rolls it back on MGC_EFORMAT)
  return rc != MGC_OK ? rc : rc_end;
}

// ---- a BGZF BAM file: mgc_push_text_bgzf_file with the record walker (mgc_bam_walk.hpp) and the device decoder (mgc_bam.hip) in the
// consumer.  The workers inflate the blocks of chunk after chunk into the ring (CRC checked); the calling thread takes the chunks in
// file order, walks each one's records -- a few bytes per record -- and queues upload + decode.  What was one host thread expanding
// every base (meryl_seq.cpp) is one host thread reading 36 bytes per record.
extern "C" int mgc_push_bam_file(mgc_session *s, const char *path, int threads) {
  if (!s || !path) return MGC_EINVAL;
  BgzfFile f;
  int rc = f.open(s, "mgc_push_bam_file", path, threads);
  if (rc != MGC_OK) return rc;
  rc = mgc_begin_bam(s);
  if (rc != MGC_OK) return rc;

  uint64_t bam_total = 0;
  bool refused = false;
  auto consume = [&](uint64_t, const char *p, size_t len) {
    bam_total += len;
    if (!len) return (int)MGC_OK;                               // (a chunk of empty blocks: the end-of-file marker)
    const int r = mgc::bam_submit(s, p, len);
    if (r == mgc::BAM_REFUSED) refused = true;
    return r;
  };
  const uint64_t nchunks = f.plan.chunks.size();
  const mgc::ChunkRingResult res = run_session_ring(s, nchunks, f.g, [&f](int t, uint64_t c, char *dst, int *bad) { return f.fill(t, c, dst, bad); }, consume);
  mgc::text_drain(s);                                           // the last uploads still read from the ring
  if (getenv("MGC_IO_TRACE"))
    fprintf(stderr, "[io] BAM file %.2f GB -> %.2f GB of records in %llu chunks (%zu blocks), %d inflaters, ring %d: waiting for the inflaters %.3f s, "
                    "walk %.3f s (%llu records), upload+decode submit (incl. the walk and waits for the device) %.3f s\n", f.fsize / 1e9, bam_total / 1e9,
            (unsigned long long)nchunks, f.plan.blocks.size(), f.g.threads, f.g.slots, res.t_wait, s->tr_bam_walk, (unsigned long long)s->bam_walker.records(), res.t_consume);
  if (res.end == mgc::ChunkRingResult::ALLOC_FAILED) { set_err(&s->err, "mgc_push_bam_file: pinned buffers: out of memory"); (void)mgc::text_rollback(s); return MGC_ENOMEM; }
  if (res.end == mgc::ChunkRingResult::FILL_FAILED) return BgzfFile::refuse_block(s, path, res.detail);
  if (refused) return mgc::bam_refuse(s, path);
  if (res.end == mgc::ChunkRingResult::CONSUMER_STOPPED) { (void)mgc::text_rollback(s); return res.detail; }
  return mgc::bam_end(s, path);                                 // a stream that ends inside a record is refused here, by the file's name
}

// ---- a plain gzip file (one deflate stream per member, no block index): mgc_gzip_par.hpp's workers inflate it from guessed block starts
// STRAIGHT into the pinned upload ring, writing markers for what they cannot know; the calling thread takes the pieces in stream order
// and queues upload -> resolve -> window -> CRC -> parse (gzip_submit).  Through the generic reader one gzread thread bounds the file.
extern "C" int mgc_is_gzip_file(const char *path) {
  if (!path) return 0;
  const int fd = open(path, O_RDONLY);
  if (fd < 0) return 0;
  unsigned char head[64];
  const ssize_t got = pread(fd, head, sizeof(head), 0);
  close(fd);
  mgc::BgzfBlock b;
  if (got < 18 || !mgc::gz_is_gzip(head, (size_t)got)) return 0;
  return mgc::bgzf_parse_block(head, (size_t)got, &b) == mgc::BGZF_NOT_BLOCK ? 1 : 0;
}

namespace {
// Compressed bytes per span.  A worker's output should fit one 32 MiB slot without a cut, and reads compress three- to six-fold:
// 4 MiB of file are 12 .. 24 MiB of text.  (A file that compresses better is cut into more pieces; nothing else changes.)  Smaller
// spans spend more of a worker's time in the finder and in markers (each piece's first 32 KiB and what is copied on from them).
constexpr uint64_t GZIP_SPAN_DEFAULT = 4u << 20;
uint64_t env_u64(const char *name, uint64_t dflt, uint64_t lo, uint64_t hi) {
  const char *v = getenv(name);
  if (!v || !*v) return dflt;
  const uint64_t x = strtoull(v, nullptr, 10);
  return std::min(std::max(x, lo), hi);
}
}  // namespace

extern "C" int mgc_push_text_gzip_file(mgc_session *s, const char *path, int format, int threads, mgc_gzip_info *info) {
  if (!s || !path) return MGC_EINVAL;
  if (info) memset(info, 0, sizeof(*info));
  uint64_t fsize = 0;
  const int fd = open_regular(&s->err, "mgc_push_text_gzip_file", path, "regular file", 0, &fsize);
  if (fd < 0) return MGC_EINVAL;
  if (fsize < 18) { close(fd); set_err(&s->err, "'%s' is not a gzip file (%llu bytes)", path, (unsigned long long)fsize); return MGC_EFORMAT; }
  const unsigned char *map = reinterpret_cast<const unsigned char *>(mmap(nullptr, fsize, PROT_READ, MAP_SHARED, fd, 0));
  if (map == MAP_FAILED) { close(fd); set_err(&s->err, "mgc_push_text_gzip_file: mmap of '%s' failed: %s", path, strerror(errno)); return MGC_EINVAL; }
  auto release = [&]() { munmap(const_cast<unsigned char *>(map), fsize); close(fd); };
  if (!mgc::gz_is_gzip(map, fsize)) { release(); set_err(&s->err, "'%s' is not a gzip file", path); return MGC_EFORMAT; }
  if (format != 0 && !known_format(format)) { release(); return MGC_EINVAL; }

  mgc::GzOptions opt;
  opt.span = env_u64("MGC_GZIP_SPAN", GZIP_SPAN_DEFAULT, 4096, 1ull << 40);
  opt.cap = env_u64("MGC_GZIP_TEXT_CAP", mgc_session::TEXT_CHUNK, 65536, mgc_session::TEXT_CHUNK);
  const mgc::ChunkRingGeometry g = mgc::chunk_ring_geometry(threads, std::max<uint64_t>(1, fsize / opt.span), mgc_session::TEXT_RING_MAX);
  opt.threads = g.threads; opt.n_slots = g.slots; opt.lag = 2;

  bool begun = false, refused = false, bad_format = false;
  char first = 0;
  int rc = MGC_OK;
  auto begin = [&](const char *text, size_t len) -> int {       // the first piece with text: it starts at a member's header, so it is exact
    if (format == 0) {
      first = first_text_byte(reinterpret_cast<const unsigned char *>(text), len);
      format = format_of(first ? first : '>');
      if (!format) { bad_format = true; return MGC_EFORMAT; }
    }
    int r = mgc_begin_text(s, format);
    if (r == MGC_OK) r = mgc::gzip_begin(s);
    begun = r == MGC_OK;
    return r;
  };
  auto consume = [&](const mgc::GzPieceView &v) -> int {
    if (!begun) {
      if (v.n_symbols) return MGC_EINVAL;                       // (cannot be: nothing precedes the first text)
      if (v.text_len == 0) {                                    // empty members in front: their trailers must say so
        for (size_t i = 0; i < v.n_ends; i++)
          if (v.ends[i].crc != 0 || v.ends[i].isize != 0) {
            char msg[120];
            snprintf(msg, sizeof(msg), "CRC32 / ISIZE mismatch (an empty member, trailer at compressed offset %llu)", (unsigned long long)v.ends[i].comp_off);
            s->gz.verdict = msg; refused = true;
            return mgc::GZIP_REFUSED;
          }
        mgc::text_drain(s);
        return MGC_OK;
      }
      const int r = begin(v.text, v.text_len);                  // (text of white space only: FASTA, as for a plain file)
      if (r != MGC_OK) return r;
    }
    const int r = mgc::gzip_submit(s, v.text, v.text_len, v.symbols, v.n_symbols, v.window_valid, v.ends, v.n_ends, v.comp_off);
    if (r == mgc::GZIP_REFUSED) refused = true;
    return r;
  };
  const mgc::GzResult res = mgc::gz_run(map, fsize, opt, s->in.file_slots, slot_alloc(s), consume);
  if (begun && !refused && res.end == mgc::GzResult::DONE && mgc::gzip_finish(s) != MGC_OK) refused = true;
  mgc::text_drain(s);                                           // the last uploads still read from the ring
  release();
  if (info) {
    info->members = res.info.members; info->chunks = res.info.chunks; info->confirmed = res.info.confirmed; info->discarded = res.info.discarded;
    info->text_bytes = res.info.text_bytes; info->symbol_bytes = res.info.symbol_bytes; info->cuts = res.info.cuts;
  }
  if (getenv("MGC_IO_TRACE"))
    fprintf(stderr, "[io] gzip %sfile %.2f GB -> %.2f GB of text (%.2f GB of symbols) in %llu chunks (%llu confirmed, %llu discarded, %llu cuts), %d inflaters, "
                    "ring %d: waiting for the inflaters %.3f s, upload+resolve+parse submit (incl. waits for the device) %.3f s; inflaters: finder %.3f s, "
                    "inflate %.3f s, waiting for a candidate %.3f s, waiting for a free slot %.3f s; of the submit: symbol copy %.3f s, CRC fold %.3f s, "
                    "waiting for the device %.3f s\n", format == MGC_TEXT_SAM ? "SAM " : "", fsize / 1e9, res.info.text_bytes / 1e9,
            res.info.symbol_bytes / 1e9, (unsigned long long)res.info.chunks, (unsigned long long)res.info.confirmed, (unsigned long long)res.info.discarded,
            (unsigned long long)res.info.cuts, opt.threads, opt.n_slots, res.t_wait, res.t_consume, res.t_find, res.t_inflate, res.t_confirm, res.t_slot_wait, s->tr_gz_copy, s->tr_gz_collect, s->tr_gz_wait);
  if (res.end == mgc::GzResult::ALLOC_FAILED) {
    set_err(&s->err, "mgc_push_text_gzip_file: pinned buffers: out of memory");
    if (begun) (void)mgc::text_rollback(s);
    return MGC_ENOMEM;
  }
  if (bad_format) { set_err(&s->err, "'%s' is neither FASTA nor FASTQ (record starts with '%c')", path, first ? first : '?'); return MGC_EFORMAT; }
  if (res.end == mgc::GzResult::FORMAT) {
    char why[200];
    snprintf(why, sizeof(why), "damaged gzip stream at compressed offset %llu (%s)", (unsigned long long)res.offset, mgc::gz_err_text(res.detail));
    if (begun) return mgc::gzip_refuse(s, path, why);
    set_err(&s->err, "'%s': %s", path, why);
    return MGC_EFORMAT;
  }
  if (refused && !begun) { set_err(&s->err, "'%s': %s", path, s->gz.verdict.c_str()); return MGC_EFORMAT; }
  if (refused) return mgc::gzip_refuse(s, path, s->gz.verdict.c_str());
  if (res.end == mgc::GzResult::CONSUMER_STOPPED) {             // a HIP error, or the worker thread's
    rc = res.detail;
    if (begun) (void)mgc::text_rollback(s);
    return rc;
  }
  if (!begun) {                                                 // no text at all: an empty file of the format asked for (FASTA when unknown)
    rc = mgc_begin_text(s, format ? format : MGC_TEXT_FASTA);
    if (rc != MGC_OK) return rc;
  }
  return mgc_end_text(s);                                       // closes the file in every case (rolls it back on MGC_EFORMAT)
}
