// reads_parse_check.cpp -- the host-side check of the FASTA / FASTQ parser (covest_amd/csrc/reads_parse.h; DESIGN.md
// section 6t), compiled and run by tests/test_reads_parse_cpu.py with the host compiler under
// -fsanitize=address,undefined.  Every input is parsed from a heap block of exactly its length, without a terminator: a
// read one byte past the end is a sanitizer report.  Each input is built record by record, so where its records start
// and end and what they spell is known here without the parser; beside it stands what the reader has to make of it.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "reads_parse.h"

using namespace covest::reads_parse;

#define CHECK(cond, ...)                                          \
    do {                                                          \
        if (!(cond)) {                                            \
            std::printf("FAILED %s:%d %s: ", __FILE__, __LINE__, #cond); \
            std::printf(__VA_ARGS__);                             \
            std::printf("\n");                                    \
            std::exit(1);                                         \
        }                                                         \
    } while (0)

struct Expect { // reads (ok), or the error and the byte it names
    bool ok = true;
    Outcome what = Outcome::kReady;
    size_t at = 0;
};
struct Input {
    std::string name;
    bool fastq = false;
    std::string text;
    std::vector<std::string> raw;     // the records' sequences as written (white space and N included)
    std::vector<size_t> starts, ends; // the records' extents
    Expect reader;                    // what the reader makes of the whole file, 4-line parser first
    Expect general;                   // FASTQ: what the general grammar makes of it from the first byte on
    int looks_wrapped = 0;            // FASTQ: the first look's answer
    bool hands_over = false;          // the 4-line parser hands over somewhere inside: batch ends are not pinned
    bool any_cut = true;              // an error that every cut of the file reports alike
    Input(const char *n, bool fq) : name(n), fastq(fq) {}
    Input &rec(const std::string &t, const std::string &seq)
    {
        starts.push_back(text.size());
        text += t;
        ends.push_back(text.size());
        raw.push_back(seq);
        return *this;
    }
    Input &other(const std::string &t) { return text += t, *this; }
    Input &fails(Outcome what, size_t at) { return reader = general = Expect{false, what, at}, *this; }
    Input &general_fails(Outcome what, size_t at) { return general = Expect{false, what, at}, *this; }
    Input &wrapped() { return looks_wrapped = 1, *this; }
    Input &wraps_later() { return hands_over = true, *this; }
};

static std::string want_read(const std::string &raw, int strategy) // preprocess, bin/kmer_hist.py:44-54 (RANDOM: 'a' stands in)
{
    std::string out;
    for (char c : raw) {
        if (std::strchr("acgtACGT", c))
            out += (char)(c | 0x20);
        else if ((c == 'n' || c == 'N') && strategy != 0)
            out += strategy == 1 ? 'a' : '?';
    }
    return out;
}

// The reader's loop without its threads and batches: spans from `pos` on until the file ends or an error stands.
struct Run {
    std::vector<std::string> reads;
    std::vector<size_t> stops;     // where each batch ended
    std::vector<bool> by_general;  // ... and which grammar read it
    Verdict v{Outcome::kReady, nullptr};
};
static Run drive(const Input &in, const ParseRules &r, bool general, int64_t max_bases, int n_threads)
{
    Run run;
    const uint8_t *strict_malformed = nullptr, *strict_bad = nullptr, *end = r.map + r.size;
    std::vector<Piece> pieces;
    for (size_t pos = 0; pos < r.size;) {
        const Span span = general ? Span{nullptr, {r.map + pos, end}} : cut_span(r, pos, max_bases, n_threads);
        const size_t n = span.cuts.size() - 1;
        if (pieces.size() < n)
            pieces.resize(n);
        const uint8_t *stop = span.stop;
        for (size_t i = 0; i < n; ++i) {
            pieces[i].clear();
            CHECK(span.cuts[i] <= span.cuts[i + 1], "%s: cuts not monotone", in.name.c_str());
            if (!general)
                parse_piece(r, span.cuts[i], span.cuts[i + 1], pieces[i]);
        }
        if (general)
            stop = parse_fastq_general(r, r.map + pos, end, pieces[0], max_bases);
        else
            CHECK(n >= 1 && n <= (size_t)n_threads && span.cuts[0] == r.map + pos && span.cuts[n] == stop && stop > r.map + pos && stop <= end,
                  "%s: span", in.name.c_str());
        const Verdict v = judge(r, general, strict_malformed, strict_bad, pieces.data(), n);
        if (v.what == Outcome::kSwitchMalformed || v.what == Outcome::kSwitchBad) {
            CHECK(!general && r.fastq, "%s: a switch out of the general grammar or in FASTA", in.name.c_str());
            (v.what == Outcome::kSwitchMalformed ? strict_malformed : strict_bad) = v.at;
            general = true;
            continue;
        }
        if (v.what != Outcome::kReady) {
            run.v = v;
            return run;
        }
        CHECK(stop && stop > r.map + pos && stop <= end, "%s: no progress", in.name.c_str());
        for (size_t i = 0; i < n; ++i) {
            size_t at = 0;
            for (int64_t len : pieces[i].lens) {
                CHECK(len >= 0 && at + (size_t)len <= pieces[i].bases.n, "%s: lengths beyond the bases", in.name.c_str());
                run.reads.emplace_back(reinterpret_cast<const char *>(pieces[i].bases.p) + at, (size_t)len);
                at += (size_t)len;
            }
            CHECK(at == pieces[i].bases.n, "%s: bases outside every read", in.name.c_str());
        }
        pos = (size_t)(stop - r.map);
        run.stops.push_back(pos);
        run.by_general.push_back(general);
        if (strict_malformed && stop > strict_malformed)
            strict_malformed = nullptr;
        if (strict_bad && stop > strict_bad)
            strict_bad = nullptr;
    }
    return run;
}

static void check_outcome(const Input &in, const Expect &want, const Run &run, const ParseRules &r, int strategy, const char *how)
{
    if (!want.ok) {
        CHECK(run.v.what == want.what && run.v.at == r.map + want.at, "%s (%s): verdict %d at %ld, wanted %d at %zu", in.name.c_str(), how,
              (int)run.v.what, run.v.at ? (long)(run.v.at - r.map) : -1, (int)want.what, want.at);
        CHECK(!message(r, run.v).empty() && message(r, run.v).find("covest_reads_next: ") == 0, "%s: message", in.name.c_str());
        return;
    }
    CHECK(run.v.what == Outcome::kReady, "%s (%s): verdict %d at %ld, wanted reads", in.name.c_str(), how, (int)run.v.what,
          run.v.at ? (long)(run.v.at - r.map) : -1);
    CHECK(run.reads.size() == in.raw.size(), "%s (%s): %zu reads, wanted %zu", in.name.c_str(), how, run.reads.size(), in.raw.size());
    for (size_t i = 0; i < in.raw.size(); ++i) {
        const std::string want_i = want_read(in.raw[i], strategy);
        bool same = run.reads[i].size() == want_i.size();
        for (size_t k = 0; same && k < want_i.size(); ++k)
            same = want_i[k] == '?' ? std::strchr("acgt", run.reads[i][k]) != nullptr : want_i[k] == run.reads[i][k];
        CHECK(same, "%s (%s, N strategy %d): read %zu is '%s'", in.name.c_str(), how, strategy, i, run.reads[i].c_str());
    }
}

// Where the batches have to end, from the records' extents alone.  4-line parser and FASTA: the first record that starts
// at or after begin + max(1, min(rest, max_bases * per_base + 64)), per_base 2.1 (FASTQ) and 1.08; the end of the file
// if there is none.  General grammar: behind the record with which max_bases bases are reached.
static void check_stops(const Input &in, const Run &run, int64_t max_bases, int strategy, const char *how)
{
    const size_t size = in.text.size();
    size_t pos = 0, i = 0; // i: the first record that can matter (the batches go forward)
    for (size_t s = 0; s < run.stops.size(); ++s) {
        size_t want = size;
        if (!run.by_general[s]) {
            const double bytes = std::min<double>((double)(size - pos), (double)max_bases * (in.fastq ? 2.1 : 1.08) + 64.0);
            const size_t from = pos + std::max<size_t>((size_t)bytes, 1);
            while (i < in.starts.size() && in.starts[i] < from)
                ++i;
            if (i < in.starts.size())
                want = in.starts[i];
        } else {
            while (i < in.starts.size() && in.starts[i] < pos)
                ++i;
            int64_t bases = 0;
            for (size_t k = i; k < in.starts.size() && want == size; ++k)
                if ((bases += (int64_t)want_read(in.raw[k], strategy).size()) >= max_bases)
                    want = in.ends[k];
        }
        CHECK(run.stops[s] == want, "%s (%s): batch %zu from %zu ends at %zu, wanted %zu", in.name.c_str(), how, s, pos, run.stops[s], want);
        pos = run.stops[s];
    }
    CHECK(pos == size, "%s (%s): the batches end at %zu of %zu", in.name.c_str(), how, pos, size);
}

static uint8_t *exact_copy(const std::string &text) // a heap block of exactly the text's length, no terminator
{
    uint8_t *block = new uint8_t[text.size()];
    if (!text.empty())
        std::memcpy(block, text.data(), text.size());
    return block;
}

static void check_input(const Input &in)
{
    uint8_t *block = exact_copy(in.text);
    for (int strategy = 0; strategy < 3; ++strategy) {
        const ParseRules r{in.fastq, strategy, 12345, block, in.text.size()};
        const bool wrapped = in.fastq && r.size && fastq_looks_wrapped(r);
        CHECK(!in.fastq || wrapped == (bool)in.looks_wrapped, "%s: looks wrapped %d", in.name.c_str(), (int)wrapped);
        const Run whole = drive(in, r, wrapped, (int64_t)1 << 40, 1);
        check_outcome(in, in.reader, whole, r, strategy, "whole");
        if (in.fastq) {
            const Run general = drive(in, r, true, (int64_t)1 << 40, 1);
            check_outcome(in, in.general, general, r, strategy, "general grammar");
            CHECK(!in.general.ok || !in.reader.ok || general.reads == whole.reads, "%s: the grammars differ", in.name.c_str());
        }
        for (int threads : {1, 3, 16}) {
            for (int64_t max_bases : {(int64_t)1, (int64_t)1000, (int64_t)1 << 22}) {
                const std::string how = std::to_string(threads) + " threads, max_bases " + std::to_string((long long)max_bases);
                const Run cut = drive(in, r, wrapped, max_bases, threads);
                if (in.reader.ok || in.any_cut)
                    check_outcome(in, in.reader, cut, r, strategy, how.c_str());
                if (in.reader.ok) {
                    CHECK(cut.reads == whole.reads, "%s (%s): the cut parse differs from the whole", in.name.c_str(), how.c_str());
                    if (!in.hands_over)
                        check_stops(in, cut, max_bases, strategy, how.c_str());
                }
            }
        }
    }
    delete[] block;
}

// next_record at every byte offset: the first record that starts at or after it (offset 0: the file's start).
static void probe_next_record(const Input &in)
{
    uint8_t *block = exact_copy(in.text);
    const ParseRules r{in.fastq, 0, 0, block, in.text.size()};
    for (size_t off = 0; off <= r.size; ++off) {
        size_t want = off == 0 ? 0 : r.size;
        for (size_t i = 0; i < in.starts.size() && want == r.size; ++i)
            if (in.starts[i] >= off)
                want = in.starts[i];
        const size_t got = (size_t)(next_record(r, block + off) - block);
        CHECK(got == want, "%s: next_record(%zu) = %zu, wanted %zu", in.name.c_str(), off, got, want);
    }
    delete[] block;
}

static uint64_t g_state = 7;
static unsigned draw(unsigned n) { return (unsigned)((g_state = mix64(g_state + 0x9E3779B97F4A7C15ull)) % n); }
static std::string letters(size_t n, const char *from)
{
    std::string s(n, 'a');
    for (char &c : s)
        c = from[draw((unsigned)std::strlen(from))];
    return s;
}

static std::vector<Input> fasta_inputs()
{
    std::vector<Input> v;
    v.emplace_back("empty.fa", false);
    v.emplace_back("header_only.fa", false).rec(">h", "");
    v.emplace_back("header_line.fa", false).rec(">h\n", "");
    v.emplace_back("no_trailing_newline.fa", false).rec(">a\nACGT\n", "ACGT").rec(">b\nGG", "GG");
    v.emplace_back("crlf.fa", false).rec(">a\r\nACGT\r\nAC\r\n", "ACGTAC").rec(">b\r\nGn\r\n", "Gn");
    v.emplace_back("text_first.fa", false).other("text before the first header\nACGT\n").rec(">r1 some description\nACGTNACGTACG\r\nTTTGACA\n", "ACGTNACGTACGTTTGACA")
        .rec(">empty\n", "").rec(">r2\nNNACGTACGTAC", "NNACGTACGTAC");
    v.emplace_back("empty_records.fa", false).rec(">a\n", "").rec(">b\n", "").rec(">c\nAC\n\n", "AC").rec(">d\n", "");
    v.emplace_back("no_header.fa", false).other("no header anywhere\nACGT\n");
    v.emplace_back("bad_base.fa", false).rec(">x\nACGT\nACRT\n", "").fails(Outcome::kBadBase, 10);
    // the 16-byte block of put_line and its remainder: an N, a space, a letter outside acgtn at the first, 16th and last place
    Input lines("line_lengths.fa", false);
    for (size_t len : {15, 16, 17, 31, 32, 33}) {
        lines.rec(">clean\n" + std::string(len, 'G') + "\n", std::string(len, 'G'));
        for (size_t place : {(size_t)0, (size_t)15, len - 1}) {
            if (place >= len)
                continue;
            for (char c : {'N', 'n', ' ', 'X'}) {
                std::string line = letters(len, "ACGTacgt");
                line[place] = c;
                if (c != 'X') {
                    lines.rec(">r\n" + line + "\n", line);
                    continue;
                }
                v.emplace_back(("bad_letter_" + std::to_string(len) + "_" + std::to_string(place) + ".fa").c_str(), false)
                    .rec(">ok\nAC\n", "AC").rec(">r\n" + line, "").fails(Outcome::kBadBase, 7 + 3 + place);
            }
        }
    }
    v.push_back(lines);
    Input big("ragged_3MiB.fa", false); // more than one piece for 3 and 16 threads
    while (big.text.size() < (size_t)3 << 20) {
        const std::string seq = letters(draw(500), draw(8) ? "ACGTacgt" : "ACGTNn");
        std::string t = ">read " + std::string(draw(40), 'x') + "\n";
        for (size_t a = 0; a < seq.size(); a += 70)
            t += seq.substr(a, 70) + "\n";
        big.rec(t, seq);
    }
    v.push_back(big);
    return v;
}

static std::vector<Input> fastq_inputs()
{
    std::vector<Input> v;
    const auto plain = [](Input &in, int n) {
        for (int i = 0; i < n; ++i)
            in.rec("@p" + std::to_string(i) + "\nACGTACGTAC\n+\nIIIIIIIIII\n", "ACGTACGTAC");
    };
    v.emplace_back("empty.fq", true);
    v.emplace_back("header_only.fq", true).general_fails(Outcome::kMalformed, 0).other("@h"); // (4-line parser: no sequence line, no read)
    v.emplace_back("ends_in_sequence.fq", true).rec("@r\nACGT", "ACGT").general_fails(Outcome::kMalformed, 0);
    v.emplace_back("blank_lines.fq", true).rec("@a\nACGT\n+\nIIII\n", "ACGT").other("\n\n").rec("@b\nTTGN\n+\n@III\n", "TTGN").other("\r\n")
        .rec("@c\nGG\n+\n+I\n", "GG").rec("@d\nAC\n+\nII\n", "AC").other("\n\n\n");
    v.emplace_back("crlf.fq", true).rec("@a\r\nACGT\r\n+\r\nIIII\r\n", "ACGT").other("\r\n").rec("@b\r\nGG\r\n+\r\nII\r\n", "GG");
    v.emplace_back("wrapped_sequence.fq", true).wrapped().rec("@a\nACNN\nNGT\n+\nIIII\nIII\n", "ACNNNGT").other("\n").rec("@b\nAC\n+\n@I\n", "AC");
    v.emplace_back("wrapped_quality.fq", true).wrapped().rec("@a\nACGTACGT\n+\nIIII\n@III\n", "ACGTACGT").rec("@x\nTTTTGGGG\n+\nIIIIIIII\n", "TTTTGGGG");
    Input advice("quality_wraps_late.fq", true); // 400 plain records, then only the QUALITY wraps and its second line starts with '@'
    plain(advice, 400);
    advice.wraps_later().rec("@w\nACGTACGT\n+\nIIII\n@III\n", "ACGTACGT").rec("@x\nTTTTGGGG\n+\nIIIIIIII\n", "TTTTGGGG");
    v.push_back(advice);
    Input stands("quality_wraps_late_and_short.fq", true); // ... and no grammar reads the rest: the 4-line parser's complaint stands
    plain(stands, 400);
    stands.wraps_later().rec("@w\nACGTACGT\n+\nIIII\n@III\n", "").other("@x\nTTTTGGGG\n+\nIII\n");
    stands.reader = Expect{false, Outcome::kBadBase, stands.ends.back()};      // '@' of "@x", taken for a base
    stands.general = Expect{false, Outcome::kMalformed, stands.ends.back()};   // the record "@x", its quality too short
    stands.any_cut = false; // (cut at "@x", a record start by its looks, the 4-line parser reads both halves)
    v.push_back(stands);
    Input late("sequence_wraps_late.fq", true); // the third line is no '+': handed over at a malformed line
    plain(late, 300);
    late.wraps_later().rec("@w\nACGT\nACGT\n+\nIIIIIIII\n", "ACGTACGT").rec("@y\nGG\n+\nII\n", "GG");
    v.push_back(late);
    v.emplace_back("ends_in_wrapped_sequence.fq", true).wrapped().rec("@a\nACGT\nAC\n+\nIIIIII\n", "").other("@b\nAC\nGT").fails(Outcome::kMalformed, 20);
    v.emplace_back("ends_in_quality.fq", true).wrapped().other("@a\nACGT\nACGT\n+\nIIIIII\n").fails(Outcome::kMalformed, 0);
    v.emplace_back("quality_too_long.fq", true).other("@a\nACGT\n+\nIIII\nII\n@b\nAC\n+\nII\n").fails(Outcome::kMalformedEitherWay, 15).general_fails(Outcome::kMalformed, 15);
    v.emplace_back("first_line_without_at.fq", true).other("ACGT\n+\nIIII\n").fails(Outcome::kMalformedEitherWay, 0).general_fails(Outcome::kMalformed, 0);
    v.emplace_back("third_line_without_plus.fq", true).other("@a\nACGT\n\nIIII\n").fails(Outcome::kMalformedEitherWay, 8).general_fails(Outcome::kBadBase, 9);
    v.emplace_back("bad_base_strict.fq", true).other("@x\nACGU\n+\nIIII\n").fails(Outcome::kBadBase, 6);
    v.emplace_back("bad_base_general.fq", true).wrapped().other("@a\nACGT\nAXGT\n+\nIIIIIIII\n").fails(Outcome::kBadBase, 9);
    Input big("plain_3MiB.fq", true); // more than one piece; qualities that open with '@' and '+'
    for (int i = 0; big.text.size() < (size_t)3 << 20; ++i) {
        const std::string seq = letters(1 + draw(200), draw(8) ? "ACGT" : "ACGTN");
        big.rec("@r\n" + seq + "\n+\n" + (i % 3 ? "@" : "+") + std::string(seq.size() - 1, 'I') + "\n", seq);
    }
    v.push_back(big);
    return v;
}

int main()
{
    const std::vector<Input> fasta = fasta_inputs(), fastq = fastq_inputs();
    for (const Input &in : fasta)
        check_input(in);
    for (const Input &in : fastq)
        check_input(in);
    for (const Input &in : fasta)
        if (in.name == "text_first.fa" || in.name == "empty_records.fa")
            probe_next_record(in);
    for (const Input &in : fastq)
        if (in.name == "blank_lines.fq")
            probe_next_record(in);
    std::printf("reads_parse_check ok: %zu FASTA and %zu FASTQ inputs\n", fasta.size(), fastq.size());
    return 0;
}
