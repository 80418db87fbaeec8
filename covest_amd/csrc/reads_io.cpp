// reads_io.cpp -- the file front-end of the k-mer histogram: FASTA / FASTQ records to the
// packed {bases, offsets} batches covest_kmer_add takes.  What turns bytes into bases and lengths is reads_parse.h (the
// reference restated there); here is what needs the process: the handle, the mapping, the batches and the threads.
// The file is mapped, a batch is a span of it that ends on a record boundary, the span is cut at record boundaries into
// one piece per thread, every piece is parsed by a table-driven pass over its bytes, and the pieces are copied side by
// side into the batch -- which lives in page-locked memory when the process has a HIP device, so that
// covest_kmer_add's copy to the device runs at the speed of the bus.  Two batch buffers alternate: a batch stays
// valid while the next one is being produced (a caller can parse batch i + 1 while the GPU counts batch i).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include "../../include/covest_amd.h"
#include "reads_parse.h"

namespace covest {
int set_error(int code, const std::string &msg); // host_common.cpp: records the message for covest_last_error
}

using namespace covest::reads_parse;

namespace {

// a batch handed to the caller: page-locked when a HIP device is there, plain memory otherwise
struct Batch {
    uint8_t *bases = nullptr;
    size_t cap = 0;
    bool pinned = false;
    std::vector<int64_t> offsets;
    void release()
    {
        if (bases) {
            if (pinned)
                (void)hipHostFree(bases);
            else
                std::free(bases);
        }
        bases = nullptr;
        cap = 0;
    }
    bool reserve(size_t n, bool want_pinned)
    {
        if (n <= cap)
            return true;
        release();
        size_t c = (size_t)1 << 20;
        while (c < n)
            c *= 2;
        if (want_pinned && hipHostMalloc(reinterpret_cast<void **>(&bases), c, hipHostMallocDefault) == hipSuccess) {
            pinned = true;
        } else {
            (void)hipGetLastError();
            bases = static_cast<uint8_t *>(std::malloc(c));
            pinned = false;
        }
        cap = bases ? c : 0;
        return bases != nullptr;
    }
};

} // namespace

struct covest_reads {
    int fd = -1;
    ParseRules rules;
    size_t pos = 0;       // the next unparsed byte -- the file's start, or a record's first byte
    bool wrapped = false; // FASTQ whose sequence / quality run over several lines (Bio.SeqIO reads those too): the general
                          // grammar, one record after the other, single-threaded (see parse_fastq_general)
    const uint8_t *strict_malformed = nullptr; // where the 4-line parser gave up and handed over to the general grammar
    const uint8_t *strict_bad = nullptr;       // ... or the "base" it refused there (a quality line it took for a sequence)
    int n_threads = 1;
    bool want_pinned = false;
    Batch batch[2];
    int cur = 0;
    std::vector<Piece> pieces; // the threads' buffers, kept from batch to batch (their pages stay touched)
    ~covest_reads()
    {
        batch[0].release();
        batch[1].release();
        if (rules.map && rules.size)
            ::munmap(const_cast<uint8_t *>(rules.map), rules.size);
        if (fd >= 0)
            ::close(fd);
    }
};

namespace {

// f(0) ... f(n - 1): in threads of their own when there is more than one
template <class F>
void each_piece(size_t n, F f)
{
    if (n == 1)
        return f(0);
    std::vector<std::thread> workers;
    for (size_t i = 0; i < n; ++i)
        workers.emplace_back(f, i);
    for (std::thread &w : workers)
        w.join();
}

// The pieces of the batch that starts at r->pos (r->pos < size), parsed: by the general grammar one piece of whole
// records until max_bases are there; else the span cut for the threads.  Returns where the batch ends (nullptr: the
// general grammar met an error, the piece says which).
const uint8_t *parse_span(covest_reads *r, int64_t max_bases, size_t &n_pieces)
{
    const ParseRules &rules = r->rules;
    const Span span = r->wrapped ? Span{nullptr, {rules.map + r->pos, rules.map + rules.size}}
                                 : cut_span(rules, r->pos, max_bases, r->n_threads);
    n_pieces = span.cuts.size() - 1;
    if (r->pieces.size() < n_pieces)
        r->pieces.resize(n_pieces);
    for (size_t i = 0; i < n_pieces; ++i)
        r->pieces[i].clear();
    if (r->wrapped)
        return parse_fastq_general(rules, span.cuts[0], span.cuts[1], r->pieces[0], max_bases);
    each_piece(n_pieces, [&](size_t i) { parse_piece(rules, span.cuts[i], span.cuts[i + 1], r->pieces[i]); });
    return span.stop;
}

// The pieces side by side into the batch: bases copied (in parallel), lengths turned into offsets.  Returns the reads.
int64_t place(const std::vector<Piece> &pieces, size_t n_pieces, Batch &out, bool want_pinned)
{
    std::vector<size_t> base_at(n_pieces + 1, 0), rec_at(n_pieces + 1, 0);
    for (size_t i = 0; i < n_pieces; ++i) {
        base_at[i + 1] = base_at[i] + pieces[i].bases.n;
        rec_at[i + 1] = rec_at[i] + pieces[i].lens.size();
    }
    if (!out.reserve(std::max<size_t>(base_at[n_pieces], 1), want_pinned))
        throw std::bad_alloc();
    out.offsets.resize(rec_at[n_pieces] + 1);
    each_piece(n_pieces, [&](size_t i) {
        const Piece &pc = pieces[i];
        if (pc.bases.n)
            std::memcpy(out.bases + base_at[i], pc.bases.p, pc.bases.n);
        int64_t at = (int64_t)base_at[i];
        int64_t *o = out.offsets.data() + rec_at[i];
        for (size_t k = 0; k < pc.lens.size(); ++k) {
            at += pc.lens[k];
            o[k + 1] = at;
        }
    });
    return (int64_t)rec_at[n_pieces];
}

} // namespace

extern "C" {

int covest_reads_open(const char *path, int32_t n_strategy, uint64_t seed, covest_reads **out)
{
    if (!path || !out)
        return covest::set_error(COVEST_E_INVALID, "covest_reads_open: null argument");
    if (n_strategy < 0 || n_strategy > 2)
        return covest::set_error(COVEST_E_INVALID, "covest_reads_open: invalid N strategy (0 IGNORE, 1 SINGLE, 2 RANDOM)");
    const int fd = ::open(path, O_RDONLY);
    if (fd < 0)
        return covest::set_error(COVEST_E_INVALID, std::string("covest_reads_open: cannot open ") + path);
    struct stat st;
    if (::fstat(fd, &st) != 0 || !S_ISREG(st.st_mode)) {
        ::close(fd);
        return covest::set_error(COVEST_E_INVALID, std::string("covest_reads_open: not a regular file: ") + path);
    }
    covest_reads *r = new (std::nothrow) covest_reads;
    if (!r) {
        ::close(fd);
        return covest::set_error(COVEST_E_NOMEM, "covest_reads_open: out of host memory");
    }
    r->fd = fd;
    r->rules.size = (size_t)st.st_size;
    if (r->rules.size) {
        void *m = ::mmap(nullptr, r->rules.size, PROT_READ, MAP_PRIVATE, fd, 0);
        if (m == MAP_FAILED) {
            delete r;
            return covest::set_error(COVEST_E_INVALID, std::string("covest_reads_open: cannot map ") + path);
        }
        r->rules.map = static_cast<const uint8_t *>(m);
        (void)::madvise(m, r->rules.size, MADV_SEQUENTIAL);
    }
    const char *dot = std::strrchr(path, '.');
    const char *slash = std::strrchr(path, '/');
    if (dot && (!slash || dot > slash))
        r->rules.fastq = std::strcmp(dot, ".fq") == 0 || std::strcmp(dot, ".fastq") == 0;
    r->rules.n_strategy = n_strategy;
    r->rules.seed = seed;
    r->wrapped = r->rules.fastq && r->rules.size && fastq_looks_wrapped(r->rules);
    // threads: COVEST_READER_THREADS, or what the machine offers, 16 at most
    unsigned hw = std::thread::hardware_concurrency();
    int nt = hw ? (int)std::min(hw, 16u) : 4;
    if (const char *e = std::getenv("COVEST_READER_THREADS"))
        nt = std::max(1, std::atoi(e));
    r->n_threads = nt;
    // page-locked batches when the process has a HIP device (COVEST_READER_PINNED=0: never)
    int n_dev = 0;
    const char *pin = std::getenv("COVEST_READER_PINNED");
    r->want_pinned = !(pin && std::atoi(pin) == 0) && hipGetDeviceCount(&n_dev) == hipSuccess && n_dev > 0;
    (void)hipGetLastError();
    *out = r;
    return COVEST_OK;
}

void covest_reads_close(covest_reads *r) { delete r; }

int covest_reads_next(covest_reads *r, int64_t max_bases, const uint8_t **bases, const int64_t **offsets,
                      int64_t *n_reads)
{
    if (!r || !bases || !offsets || !n_reads)
        return covest::set_error(COVEST_E_INVALID, "covest_reads_next: null argument");
    if (max_bases < 1)
        max_bases = 1;
    const ParseRules &rules = r->rules;
    Batch &out = r->batch[r->cur]; // this call's buffer, whatever happens below: the other one stays the caller's
    r->cur ^= 1;
    try {
        out.offsets.assign(1, 0);
        *bases = reinterpret_cast<const uint8_t *>("");
        *offsets = out.offsets.data();
        *n_reads = 0;
        while (*n_reads == 0 && r->pos < rules.size) { // (a span without a single record -- text before the first header: go on)
            size_t n_pieces = 0;
            const uint8_t *stop = parse_span(r, max_bases, n_pieces);
            const Verdict v = judge(rules, r->wrapped, r->strict_malformed, r->strict_bad, r->pieces.data(), n_pieces);
            if (v.what == Outcome::kSwitchMalformed || v.what == Outcome::kSwitchBad) { // the general grammar, from this batch's start
                r->wrapped = true;
                (v.what == Outcome::kSwitchMalformed ? r->strict_malformed : r->strict_bad) = v.at;
                continue;
            }
            if (v.what != Outcome::kReady)
                return covest::set_error(v.what == Outcome::kNoMemory ? COVEST_E_NOMEM : COVEST_E_INVALID, message(rules, v));
            *n_reads = place(r->pieces, n_pieces, out, r->want_pinned);
            *bases = out.bases;
            *offsets = out.offsets.data();
            r->pos = (size_t)(stop - rules.map);
            if (r->strict_malformed && stop > r->strict_malformed)
                r->strict_malformed = nullptr; // (the general grammar took what the 4-line parser could not)
            if (r->strict_bad && stop > r->strict_bad)
                r->strict_bad = nullptr;
        }
    } catch (const std::bad_alloc &) {
        return covest::set_error(COVEST_E_NOMEM, message(rules, {Outcome::kNoMemory, nullptr}));
    }
    return COVEST_OK;
}

int64_t covest_reads_bytes(const covest_reads *r) { return r ? (int64_t)r->pos : 0; }

} // extern "C"
