// reads_parse.h -- FASTA / FASTQ bytes to bases and read lengths: what the file front-end (reads_io.cpp) does without
// HIP and without its handle.  Plain C++; tests/reads_parse_check.cpp runs it under sanitizers.
// Reference restated (paths in the reference checkout):
//   load_reads   bin/kmer_hist.py:67-74   format by extension (.fq / .fastq: FASTQ, anything else FASTA), one
//                                         sequence per record (the reference delegates the parsing to Bio.SeqIO)
//   preprocess   bin/kmer_hist.py:44-54   lower case; N dropped (IGNORE), replaced by 'a' (SINGLE) or by a random
//                                         base (RANDOM)
//   single_hash  bin/kmer_hist.py:14-15   any other letter is a KeyError: here an error naming the letter
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#if defined(__SSE2__)
#include <emmintrin.h>
#endif

namespace covest {
namespace reads_parse {

enum : uint8_t { kBase = 0, kN = 1, kSpace = 2, kBad = 3 };

struct ByteClass {
    uint8_t cls[256];
    uint8_t lower[256];
    ByteClass()
    {
        for (int c = 0; c < 256; ++c) {
            cls[c] = kBad;
            lower[c] = (uint8_t)((c >= 'A' && c <= 'Z') ? c + 32 : c);
        }
        for (const char *p = "acgtACGT"; *p; ++p)
            cls[(uint8_t)*p] = kBase;
        cls[(uint8_t)'n'] = cls[(uint8_t)'N'] = kN;
        for (const char *p = " \t\r\n\v\f"; *p; ++p)
            cls[(uint8_t)*p] = kSpace;
    }
};
const ByteClass kBytes;

// a plain growable byte buffer (std::vector::resize would zero-fill every byte before it is written)
struct Bytes {
    uint8_t *p = nullptr;
    size_t n = 0, cap = 0;
    Bytes() = default;
    Bytes(const Bytes &) = delete;
    Bytes &operator=(const Bytes &) = delete;
    Bytes(Bytes &&o) noexcept : p(o.p), n(o.n), cap(o.cap) { o.p = nullptr, o.n = o.cap = 0; }
    ~Bytes() { std::free(p); }
    uint8_t *grow(size_t extra)
    {
        if (n + extra > cap) {
            size_t c = cap ? cap : (size_t)1 << 16;
            while (c < n + extra)
                c *= 2;
            uint8_t *q = static_cast<uint8_t *>(std::realloc(p, c));
            if (!q)
                throw std::bad_alloc();
            p = q;
            cap = c;
        }
        return p + n;
    }
};

// what one thread makes of its piece of the span
struct Piece {
    Bytes bases;
    std::vector<int64_t> lens;          // one per record, in file order
    const uint8_t *bad = nullptr;       // first letter single_hash would reject
    const uint8_t *malformed = nullptr; // FASTQ: first line (4-line framing) or record (general grammar) that breaks it
    bool oom = false;
    void clear() { bases.n = 0, lens.clear(), bad = malformed = nullptr, oom = false; }
};

// what the parsers read of an open file
struct ParseRules {
    bool fastq = false;
    int n_strategy = 0; // 0 IGNORE, 1 SINGLE, 2 RANDOM
    uint64_t seed = 0;
    const uint8_t *map = nullptr;
    size_t size = 0;
};

inline uint64_t mix64(uint64_t z)
{
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// The line cursor: [p, stop) is a line without its '\n' (a '\r' in front of it stays).
struct Line {
    const uint8_t *p, *stop;
    bool blank() const { return stop == p || (stop == p + 1 && *p == '\r'); }
    size_t chars() const // characters that are not white space
    {
        size_t n = 0;
        for (const uint8_t *c = p; c < stop; ++c)
            n += kBytes.cls[*c] != kSpace;
        return n;
    }
};
inline Line take_line(const uint8_t *&p, const uint8_t *e) // the line at p (p < e); p moves behind it
{
    const uint8_t *nl = static_cast<const uint8_t *>(std::memchr(p, '\n', (size_t)(e - p)));
    const Line line{p, nl ? nl : e};
    p = nl ? nl + 1 : e;
    return line;
}

// The sequence bytes [p, e) of one line into the piece.  The common case -- nothing but a/c/g/t -- is one pass that
// lower-cases into place; anything else goes byte by byte.  Returns false at a letter outside acgtn (piece.bad).
inline bool put_line(const ParseRules &r, Piece &pc, const uint8_t *p, const uint8_t *e)
{
    const size_t n = (size_t)(e - p);
    uint8_t *out = pc.bases.grow(n);
    uint8_t seen = 0;
    size_t i = 0;
#if defined(__SSE2__)
    // 16 bytes at a time: c | 0x20 lower-cases a letter; the line is clean if every byte then is one of a c g t
    const __m128i bit5 = _mm_set1_epi8(0x20), la = _mm_set1_epi8('a'), lc = _mm_set1_epi8('c'),
                  lg = _mm_set1_epi8('g'), lt = _mm_set1_epi8('t');
    __m128i all_ok = _mm_set1_epi8((char)0xFF);
    for (; i + 16 <= n; i += 16) {
        const __m128i v = _mm_or_si128(_mm_loadu_si128(reinterpret_cast<const __m128i *>(p + i)), bit5);
        const __m128i ok = _mm_or_si128(_mm_or_si128(_mm_cmpeq_epi8(v, la), _mm_cmpeq_epi8(v, lc)),
                                        _mm_or_si128(_mm_cmpeq_epi8(v, lg), _mm_cmpeq_epi8(v, lt)));
        all_ok = _mm_and_si128(all_ok, ok);
        _mm_storeu_si128(reinterpret_cast<__m128i *>(out + i), v);
    }
    if (_mm_movemask_epi8(all_ok) != 0xFFFF)
        seen = kBad; // (something else in there: sorted out byte by byte below)
#endif
    for (; i < n; ++i) {
        out[i] = kBytes.lower[p[i]];
        seen |= kBytes.cls[p[i]];
    }
    if (seen == kBase) {
        pc.bases.n += n;
        return true;
    }
    size_t w = 0;
    for (; p < e; ++p) {
        const uint8_t c = kBytes.cls[*p];
        if (c == kBase) {
            out[w++] = kBytes.lower[*p];
        } else if (c == kN) {
            if (r.n_strategy == 1)
                out[w++] = (uint8_t)'a';
            else if (r.n_strategy == 2) // a function of the seed and of WHERE the N stands: the same whatever the threads
                out[w++] = (uint8_t)"acgt"[mix64(r.seed + 0x9E3779B97F4A7C15ull * (uint64_t)(p - r.map + 1)) & 3];
            // IGNORE: dropped
        } else if (c != kSpace) {
            pc.bad = p;
            return false;
        }
    }
    pc.bases.n += w;
    return true;
}

// FASTA records of [b, e): b is the file's start (text before the first header is skipped) or a record's first byte,
// e a record's first byte or the end of the file.
inline void parse_fasta(const ParseRules &r, const uint8_t *b, const uint8_t *e, Piece &pc)
{
    bool in_record = false;
    int64_t start = 0;
    for (const uint8_t *p = b; p < e;) {
        const Line line = take_line(p, e);
        if (*line.p == '>') {
            if (in_record) // (an empty record is a read too: it counts k-mer 0, bin/kmer_hist.py:36-37)
                pc.lens.push_back((int64_t)pc.bases.n - start);
            in_record = true;
            start = (int64_t)pc.bases.n;
        } else if (in_record && !put_line(r, pc, line.p, line.stop)) {
            return;
        }
    }
    if (in_record)
        pc.lens.push_back((int64_t)pc.bases.n - start);
}

// Strict 4-line FASTQ records of [b, e) (what sequencers write, and what can be cut into pieces for the threads):
// @id / sequence / + / quality.  Blank lines between records (and at the end of the file) are skipped; a record whose
// first line does not start with '@' or whose third does not start with '+' is piece.malformed, not counted as garbage.
inline void parse_fastq4(const ParseRules &r, const uint8_t *b, const uint8_t *e, Piece &pc)
{
    int at = 0; // 0 = @id, 1 = sequence, 2 = +, 3 = quality
    for (const uint8_t *p = b; p < e;) {
        const Line line = take_line(p, e);
        const bool blank = line.blank();
        if (at == 0 && blank) // between records
            continue;
        if ((at == 0 && *line.p != '@') || (at == 2 && (blank || *line.p != '+'))) {
            pc.malformed = line.p;
            return;
        }
        if (at == 1) {
            const int64_t start = (int64_t)pc.bases.n;
            if (!put_line(r, pc, line.p, line.stop))
                return;
            pc.lens.push_back((int64_t)pc.bases.n - start);
        }
        at = (at + 1) & 3;
    }
}

inline void parse_piece(const ParseRules &r, const uint8_t *b, const uint8_t *e, Piece &pc)
{
    try {
        r.fastq ? parse_fastq4(r, b, e, pc) : parse_fasta(r, b, e, pc);
    } catch (const std::bad_alloc &) {
        pc.oom = true;
    }
}

// FASTQ by its GENERAL grammar, what the reference's Bio.SeqIO accepts: '@' header, sequence lines up to the line that
// starts with '+', then quality lines until they hold as many non-space characters as the sequence did.  Quality lines
// may start with '@' or '+', which is why record boundaries cannot be found by looking at line starts alone: such a file
// is read one record after the other, from a known record start.  This is the one reading of that grammar: one record
// (or one blank line) at p, p < e; p moves behind it; every sequence line goes to seq(line), which may refuse it.
enum class Fastq { kRecord, kBlank, kNoHeader, kRefused, kNoPlus, kQuality };
struct FastqLines { int seq = 0, qual = 0; };
template <class SeqSink>
inline Fastq fastq_record(const uint8_t *&p, const uint8_t *e, FastqLines &lines, SeqSink &&seq)
{
    Line line = take_line(p, e);
    if (line.blank())
        return Fastq::kBlank;
    if (*line.p != '@')
        return Fastq::kNoHeader;
    size_t seq_chars = 0, qual_chars = 0;
    bool plus = false;
    while (p < e) {
        line = take_line(p, e);
        if (line.p < line.stop && *line.p == '+') {
            plus = true;
            break;
        }
        ++lines.seq;
        seq_chars += line.chars();
        if (!seq(line))
            return Fastq::kRefused;
    }
    if (!plus) // the file ends inside the sequence
        return Fastq::kNoPlus;
    for (; qual_chars < seq_chars && p < e; ++lines.qual)
        qual_chars += take_line(p, e).chars();
    // shorter (the file ends) or longer (a line too many) than the sequence: kQuality
    return qual_chars == seq_chars ? Fastq::kRecord : Fastq::kQuality;
}

// Whole records of [b, e) by the general grammar into `pc` until `max_bases` bases are there (at least one record);
// returns where it stopped (a record's first byte, or e), nullptr on an error (pc.malformed / pc.bad / pc.oom say which).
inline const uint8_t *parse_fastq_general(const ParseRules &r, const uint8_t *b, const uint8_t *e, Piece &pc, int64_t max_bases)
{
    try {
        const uint8_t *p = b;
        while (p < e) {
            const uint8_t *rec = p;
            const int64_t start = (int64_t)pc.bases.n;
            FastqLines lines;
            const Fastq got = fastq_record(p, e, lines, [&](const Line &l) { return put_line(r, pc, l.p, l.stop); });
            if (got == Fastq::kBlank) // between records
                continue;
            if (got == Fastq::kRefused)
                return nullptr;
            if (got != Fastq::kRecord) {
                pc.malformed = rec;
                return nullptr;
            }
            pc.lens.push_back((int64_t)pc.bases.n - start);
            if ((int64_t)pc.bases.n >= max_bases)
                break;
        }
        return p;
    } catch (const std::bad_alloc &) {
        pc.oom = true;
        return nullptr;
    }
}

// Does the file look wrapped?  The first records (the first MiB, 256 at most) by the general grammar: one whose sequence
// or quality takes more than one line says yes.  (A file that starts with 4-line records and wraps later is caught when
// the strict parser meets the first such record: see `judge`.)
inline bool fastq_looks_wrapped(const ParseRules &r)
{
    const uint8_t *p = r.map, *e = r.map + std::min<size_t>(r.size, (size_t)1 << 20);
    for (int records = 0; p < e && records < 256;) {
        FastqLines lines;
        const Fastq got = fastq_record(p, e, lines, [](const Line &) { return true; });
        if (got == Fastq::kBlank)
            continue;
        if (got == Fastq::kNoHeader || got == Fastq::kNoPlus)
            return false; // (let the strict parser report it)
        if (lines.seq > 1 || lines.qual > 1)
            return true;
        ++records; // (a quality of another length on one line: the strict parser's business too)
    }
    return false;
}

// The first byte of the first record that starts at or after p (the end of the file if there is none).
inline const uint8_t *next_record(const ParseRules &r, const uint8_t *p)
{
    const uint8_t *end = r.map + r.size;
    if (p <= r.map)
        return r.map;
    const uint8_t mark = r.fastq ? '@' : '>';
    --p; // (a record may start exactly at p: look for the newline in front of it)
    while (p < end) {
        const uint8_t *nl = static_cast<const uint8_t *>(std::memchr(p, '\n', (size_t)(end - p)));
        if (!nl || nl + 1 >= end)
            return end;
        const uint8_t *c = nl + 1;
        if (*c == mark) {
            if (!r.fastq)
                return c;
            // FASTQ: '@' also opens quality lines.  A header is followed by the sequence line and then by '+'; a
            // quality line that starts with '@' is followed by the next header and ITS sequence line, never a '+'.
            const uint8_t *third = c;
            take_line(third, end);
            if (third < end)
                take_line(third, end);
            if (third < end && *third == '+')
                return c;
        }
        p = c;
    }
    return end;
}

// The span of one batch from `pos` (pos < size): about max_bases bases' worth of file (headers, line ends and -- FASTQ
// -- qualities on top), up to the next record boundary, one record at least; cut at record boundaries into one piece
// per thread (a piece per MiB at most).  cuts[0] is the span's begin, cuts.back() its stop.
struct Span {
    const uint8_t *stop = nullptr;
    std::vector<const uint8_t *> cuts;
};
inline Span cut_span(const ParseRules &r, size_t pos, int64_t max_bases, int n_threads)
{
    const uint8_t *begin = r.map + pos, *end = r.map + r.size;
    const double per_base = r.fastq ? 2.1 : 1.08;
    const size_t want = (size_t)std::min<double>((double)(end - begin), (double)max_bases * per_base + 64.0);
    const uint8_t *stop = next_record(r, begin + std::max<size_t>(want, 1));
    if (stop <= begin)
        stop = end;
    const size_t span = (size_t)(stop - begin);
    const size_t n = std::min<size_t>((size_t)n_threads, std::max<size_t>(1, span >> 20));
    Span s{stop, std::vector<const uint8_t *>(n + 1, begin)};
    s.cuts[n] = stop;
    for (size_t i = 1; i < n; ++i)
        s.cuts[i] = std::min(std::max(next_record(r, begin + span / n * i), s.cuts[i - 1]), stop);
    return s;
}

// The verdict over the pieces of one span, in file order (the first piece that complains is the first in the file).
// 4-line parser: a line that breaks the framing may open a file that wraps its lines from here on, and a "bad base" in a
// FASTQ file may be a QUALITY character -- where only the quality wraps and its second line starts with '@', behind more
// records than fastq_looks_wrapped reads, that line passes for a header and the next '@id' line for a sequence ("@w /
// ACGTACGT / + / IIII / @III / @x ..." is a file Bio.SeqIO reads).  Either way the general grammar decides, from this
// batch's start, and the caller keeps the place (strict_malformed, strict_bad) for the case that it has no reading
// either: it then names the line the 4-line parser stopped at, or lets that parser's complaint about the base stand.
enum class Outcome { kReady, kSwitchMalformed, kSwitchBad, kNoMemory, kMalformedEitherWay, kMalformed, kBadBase };
struct Verdict { Outcome what; const uint8_t *at; }; // at: the line, record or letter it is about
inline Verdict judge(const ParseRules &r, bool general, const uint8_t *strict_malformed, const uint8_t *strict_bad,
                     const Piece *pieces, size_t n_pieces)
{
    for (size_t i = 0; i < n_pieces; ++i) {
        const Piece &pc = pieces[i];
        if (pc.oom)
            return {Outcome::kNoMemory, nullptr};
        if (!pc.malformed && !pc.bad)
            continue;
        if (!general) {
            if (pc.malformed)
                return {Outcome::kSwitchMalformed, pc.malformed};
            return {r.fastq ? Outcome::kSwitchBad : Outcome::kBadBase, pc.bad};
        }
        if (strict_malformed)
            return {Outcome::kMalformedEitherWay, strict_malformed};
        if (pc.malformed && strict_bad)
            return {Outcome::kBadBase, strict_bad};
        if (pc.malformed)
            return {Outcome::kMalformed, pc.malformed};
        return {Outcome::kBadBase, pc.bad};
    }
    return {Outcome::kReady, nullptr};
}

// The text of a verdict that is an error (covest_last_error).
inline std::string message(const ParseRules &r, const Verdict &v)
{
    const std::string who = "covest_reads_next: ";
    if (v.what == Outcome::kNoMemory)
        return who + "out of host memory";
    if (v.what == Outcome::kBadBase)
        return who + "base '" + (char)*v.at + "' outside acgtn (single_hash raises KeyError)";
    return who + "malformed FASTQ record at byte " + std::to_string((long long)(v.at - r.map)) +
           (v.what == Outcome::kMalformedEitherWay ? " (@id, sequence, +, quality -- or wrapped: sequence lines, +, as many quality characters)"
                                                   : " (@id, sequence lines, +, as many quality characters)");
}

} // namespace reads_parse
} // namespace covest
