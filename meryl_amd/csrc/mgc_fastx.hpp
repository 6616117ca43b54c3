// mgc_fastx.hpp -- what the front ends that take whole FASTA/FASTQ files as sequences share (meryl_lookup_main.cpp,
// position_lookup_main.cpp): the text of a file through msr_read_text, and its names and bases as one stream with '.' after
// each sequence.  The including file provides die(fmt, arg) in its unnamed namespace.  Not installed.
#pragma once
#include "../../include/meryl_seq.h"

#include <cstdint>
#include <string>
#include <vector>

namespace {

// names and bases of a FASTA/FASTQ text (multi-line FASTA, four-line FASTQ; the reference reads both through
// dnaSeqFile::loadSequence, meryl-utility)
struct Seqs { std::vector<std::string> names; std::vector<uint64_t> start; std::string bases; };

void parse_text(const std::string &text, Seqs &out) {
  size_t p = 0;
  const size_t n = text.size();
  auto line = [&](size_t &a, size_t &b) {                   // next line [a, b) without its terminator; false at the end
    if (p >= n) return false;
    a = p;
    while (p < n && text[p] != '\n') p++;
    b = p;
    if (p < n) p++;
    if (b > a && text[b - 1] == '\r') b--;
    return true;
  };
  size_t a, b;
  bool have = line(a, b);
  while (have) {
    if (b == a) { have = line(a, b); continue; }
    const char c = text[a];
    if (c != '>' && c != '@') die("ERROR: sequence file: a record starts with '%s', neither '>' nor '@'.", std::string(1, c).c_str());
    size_t e = a + 1;
    while (e < b && text[e] != ' ' && text[e] != '\t') e++;
    out.names.push_back(text.substr(a + 1, e - a - 1));       // the identifier: first word of the header (dnaSeq::ident())
    out.start.push_back(out.bases.size());
    if (c == '>') {
      while ((have = line(a, b)) && !(b > a && text[a] == '>')) out.bases.append(text, a, b - a);
    } else {
      if ((have = line(a, b))) out.bases.append(text, a, b - a);
      if ((have = line(a, b))) {                              // '+' line
        if ((have = line(a, b))) have = line(a, b);           // quality line, then the next record
      }
    }
    out.bases.push_back('.');
  }
  out.start.push_back(out.bases.size());
}

// the whole text of a FASTA/FASTQ file (plain, gzip, BGZF, "-")
void read_fastx_text(const std::string &path, std::string &text) {
  msr_reader *r = msr_open(path.c_str());
  if (!r) die("ERROR: %s", msr_last_error());
  if (msr_format(r) != MSR_FORMAT_FASTX) die("ERROR: '%s' is not FASTA/FASTQ text.", path.c_str());
  std::vector<char> buf(16u << 20);
  for (;;) {
    const int64_t got = msr_read_text(r, buf.data(), buf.size());
    if (got < 0) die("ERROR: %s", msr_last_error());
    if (got == 0) break;
    text.append(buf.data(), (size_t)got);
  }
  msr_close(r);
}

}  // namespace
