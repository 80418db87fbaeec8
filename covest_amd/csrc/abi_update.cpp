// abi_update.cpp -- the eight forms of the C ABI that change a counter's table, covest_kmer_{add,remove}[_weighted][_device],
// over one path: a form is a row of the table below, an entry point one call of update_device or
// update_host with its row.  The adds go into the table of either key width (kmer_host.cpp table_count), the removals
// into the one-word table alone (kmer_remove.hip).
#include "host.h"

using namespace covest;

namespace {

// What tells the forms apart.  Every difference between an add and its removal that is not "add or remove" is a field
// here or a commented line below; DESIGN.md section 6ao lists them, none is decided here.
struct UpdateForm {
    const char *name;  // the entry point: its argument checks and its sticky check report under it
    const char *who;   // what the locked device call reports under: a host ADD reports under its device form's name
    bool remove, weighted;
    int sticky_word;   // of covest_kmer::flag: the word its kernels set
    bool wide_keys;    // keys of more than one word are accepted (the adds)
};

constexpr UpdateForm kAddDevice{"covest_kmer_add_device", "covest_kmer_add_device", false, false, kKmerOverflowWord, true};
constexpr UpdateForm kAddWeightedDevice{"covest_kmer_add_weighted_device", "covest_kmer_add_weighted_device", false, true,
                                        kKmerOverflowWord, true};
constexpr UpdateForm kAdd{"covest_kmer_add", "covest_kmer_add_device", false, false, kKmerOverflowWord, true};
constexpr UpdateForm kAddWeighted{"covest_kmer_add_weighted", "covest_kmer_add_weighted_device", false, true, kKmerOverflowWord,
                                  true};
constexpr UpdateForm kRemoveDevice{"covest_kmer_remove_device", "covest_kmer_remove_device", true, false, kKmerUnderflowWord,
                                   false};
constexpr UpdateForm kRemoveWeightedDevice{"covest_kmer_remove_weighted_device", "covest_kmer_remove_weighted_device", true, true,
                                           kKmerUnderflowWord, false};
constexpr UpdateForm kRemove{"covest_kmer_remove", "covest_kmer_remove", true, false, kKmerUnderflowWord, false};
constexpr UpdateForm kRemoveWeighted{"covest_kmer_remove_weighted", "covest_kmer_remove_weighted", true, true, kKmerUnderflowWord,
                                     false};

// The device call with the counter's lock held (the host forms hold it for their whole call: host.h KmerHostCall).
int update_locked(const UpdateForm &f, covest_kmer *c, const uint8_t *d_bases, const int64_t *d_offsets, int64_t n_reads,
                  int64_t read_len, const uint32_t *d_weights, void *stream)
{
    COVEST_TRY(fail_if(check_table_holds_keys(f.who, f.wide_keys ? 0 : c->wide, c->bulk))); // (an add: keys of any width)
    DeviceGuard dev_guard(c->device);
    COVEST_TRY(dev_guard.status());
    const hipStream_t st = static_cast<hipStream_t>(stream);
    if (f.remove)
        HIP_TRY(launch_kmer_remove(d_bases, d_offsets, n_reads, read_len, c->k, c->canonical, c->table,
                                   c->flag.as<int>() + f.sticky_word, st, d_weights));
    else // (table_count hands the kernels the counter's first sticky word: kKmerOverflowWord)
        HIP_TRY(table_count(c, d_bases, d_offsets, n_reads, read_len, d_weights, st));
    return COVEST_OK;
}

// A device form: asynchronous on `stream`; it never looks at the sticky words.
int update_device(const UpdateForm &f, covest_kmer *c, const uint8_t *d_bases, const int64_t *d_offsets, int64_t n_reads,
                  int64_t read_len, const uint32_t *d_weights, void *stream)
{
    COVEST_TRY(fail_if(check_update_device_args(f.name, c != nullptr, d_bases != nullptr, d_offsets != nullptr, n_reads, read_len)));
    if (f.weighted)
        COVEST_TRY(kmer_check_weights(f.name, d_weights, n_reads));
    std::lock_guard<std::mutex> guard(c->lock);
    return update_locked(f, c, d_bases, d_offsets, n_reads, read_len, d_weights, stream);
}

// A host form: the reads (and weights) staged into the counter, the device call, the wait, and what the sticky words say
// -- the update's own words, not KmerHostCall::close()'s: the batch is partly counted, the table can grow.
int update_host(const UpdateForm &f, covest_kmer *c, const uint8_t *bases, const int64_t *offsets, int64_t n_reads,
                const uint32_t *weights)
{
    COVEST_TRY(fail_if(check_update_host_args(f.name, c != nullptr, offsets != nullptr, n_reads)));
    if (f.weighted)
        COVEST_TRY(kmer_check_weights(f.name, weights, n_reads));
    // The key width before "no reads": a removal of no reads from a counter of wide keys is refused, an add of none never
    // is.  (bulk: with the lock held, in update_locked, and so behind the staging.)
    if (!f.wide_keys)
        COVEST_TRY(fail_if(check_table_holds_keys(f.name, c->wide, false)));
    if (n_reads == 0)
        return COVEST_OK;
    COVEST_TRY(fail_if(check_update_host_bytes(f.name, offsets[n_reads] - offsets[0], bases != nullptr)));
    KmerHostCall call(c);
    COVEST_TRY(call.open(bases, offsets, n_reads));
    if (f.weighted) {
        HIP_TRY(c->ws_weights.reserve((size_t)n_reads * sizeof(uint32_t)));
        HIP_TRY(hipMemcpy(c->ws_weights.ptr, weights, (size_t)n_reads * sizeof(uint32_t), hipMemcpyHostToDevice));
    }
    COVEST_TRY(update_locked(f, c, c->ws_bases.as<uint8_t>(), c->ws_offsets.as<int64_t>(), n_reads, 0,
                             f.weighted ? c->ws_weights.as<uint32_t>() : nullptr, nullptr));
    HIP_TRY(hipDeviceSynchronize());
    return kmer_check_overflow(c, f.name);
}

} // namespace

extern "C" {

int covest_kmer_add_device(covest_kmer *c, const uint8_t *d_bases, const int64_t *d_offsets, int64_t n_reads, int64_t read_len,
                           void *stream)
{
    return update_device(kAddDevice, c, d_bases, d_offsets, n_reads, read_len, nullptr, stream);
}

int covest_kmer_add_weighted_device(covest_kmer *c, const uint8_t *d_bases, const int64_t *d_offsets, int64_t n_reads,
                                    int64_t read_len, const uint32_t *d_weights, void *stream)
{
    return update_device(kAddWeightedDevice, c, d_bases, d_offsets, n_reads, read_len, d_weights, stream);
}

int covest_kmer_add(covest_kmer *c, const uint8_t *bases, const int64_t *offsets, int64_t n_reads)
{
    return update_host(kAdd, c, bases, offsets, n_reads, nullptr);
}

int covest_kmer_add_weighted(covest_kmer *c, const uint8_t *bases, const int64_t *offsets, int64_t n_reads,
                             const uint32_t *weights)
{
    return update_host(kAddWeighted, c, bases, offsets, n_reads, weights);
}

int covest_kmer_remove_device(covest_kmer *c, const uint8_t *d_bases, const int64_t *d_offsets, int64_t n_reads,
                              int64_t read_len, void *stream)
{
    return update_device(kRemoveDevice, c, d_bases, d_offsets, n_reads, read_len, nullptr, stream);
}

int covest_kmer_remove_weighted_device(covest_kmer *c, const uint8_t *d_bases, const int64_t *d_offsets, int64_t n_reads,
                                       int64_t read_len, const uint32_t *d_weights, void *stream)
{
    return update_device(kRemoveWeightedDevice, c, d_bases, d_offsets, n_reads, read_len, d_weights, stream);
}

int covest_kmer_remove(covest_kmer *c, const uint8_t *bases, const int64_t *offsets, int64_t n_reads)
{
    return update_host(kRemove, c, bases, offsets, n_reads, nullptr);
}

int covest_kmer_remove_weighted(covest_kmer *c, const uint8_t *bases, const int64_t *offsets, int64_t n_reads,
                                const uint32_t *weights)
{
    return update_host(kRemoveWeighted, c, bases, offsets, n_reads, weights);
}

} // extern "C"
