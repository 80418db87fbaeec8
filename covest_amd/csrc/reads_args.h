// reads_args.h -- the argument checks that entry points over packed reads share (abi_sample.cpp, abi_split.cpp; the reach
// check: abi_sim.cpp too; the forms over a counter's table), in plain C++ (DESIGN.md sections 6ag, 6aj).  No HIP in it:
// tests/reads_args_check.cpp runs it under the host compiler's sanitizers.  A check returns the status and the text of
// the message; the caller passes them to `fail` (host.h fail_if).
#pragma once
#include <cstdint>
#include <limits>
#include <string>

#include "../../include/covest_amd.h"

namespace covest {

struct ArgCheck {
    int status = COVEST_OK;
    std::string message;
};

inline ArgCheck arg_invalid(const std::string &name, const std::string &what)
{
    return ArgCheck{COVEST_E_INVALID, name + ": " + what};
}

// first_read + n_reads, and n_reads * read_len where read_len > 0 (0: reads with offsets of their own), within int64
inline ArgCheck check_reads_reach(const std::string &name, int64_t first_read, int64_t n_reads, int64_t read_len)
{
    const int64_t i64_max = std::numeric_limits<int64_t>::max();
    if (first_read > i64_max - n_reads || (read_len > 0 && n_reads > i64_max / read_len))
        return arg_invalid(name, "more reads than 64-bit offsets reach");
    return ArgCheck{};
}

// Of both forms of a call: the sizes, their 64-bit reach, and the output offsets that reads of their own lengths need.
inline ArgCheck check_reads_args(const std::string &name, bool has_offsets, int64_t n_reads, int64_t read_len,
                                 int64_t first_read, bool has_out_offsets)
{
    if (n_reads < 0 || first_read < 0)
        return arg_invalid(name, "n_reads and first_read must not be negative");
    if (!has_offsets && read_len < 0)
        return arg_invalid(name, "without offsets read_len must not be negative");
    const ArgCheck reach = check_reads_reach(name, first_read, n_reads, has_offsets ? 0 : read_len);
    if (reach.status != COVEST_OK)
        return reach;
    if (n_reads > 0 && has_offsets && !has_out_offsets)
        return arg_invalid(name, "reads of their own lengths need an array for the output offsets");
    return ArgCheck{};
}

// The device forms that walk reads against a counter's table (abi_lookup.cpp, abi_correct.cpp, abi_influence.cpp): their
// first check, the sizes, and their last, that the table holds the keys -- one word a key (`wide`: covest_kmer::wide, the
// words of a longer key) and not the partitioned path's result (`bulk`).  Each form keeps its own checks between the two.
inline ArgCheck check_table_reads_sizes(const std::string &name, bool has_offsets, int64_t n_reads, int64_t read_len)
{
    const bool bad = n_reads < 0 || (!has_offsets && (read_len < 0 || read_len >= ((int64_t)1 << 32)));
    return bad ? arg_invalid(name, "negative size, or no offsets and no read_len below 2^32") : ArgCheck{};
}
inline ArgCheck check_table_holds_keys(const std::string &name, int wide, bool bulk)
{
    if (wide)
        return ArgCheck{COVEST_E_UNSUPPORTED, name + ": k must be at most 31 (keys of one word)"};
    return bulk ? arg_invalid(name, "the counter holds a covest_kmer_count_reads_device result (its keys are not in the "
                                    "table); covest_kmer_clear first") : ArgCheck{};
}

// The eight forms that change a counter's table, covest_kmer_{add,remove}[_weighted][_device] (abi_update.cpp): what a
// form is given, as flags.  A device form needs its bases where it has reads and a length where it has no offsets; a
// host form needs its offsets where it has reads, and -- once it has read them: n_bytes = offsets[n_reads] - offsets[0]
// -- bytes that do not descend, with bases where there are any.
inline ArgCheck check_update_device_args(const std::string &name, bool has_counter, bool has_bases, bool has_offsets,
                                         int64_t n_reads, int64_t read_len)
{
    const bool bad = !has_counter || n_reads < 0 || (n_reads > 0 && !has_bases) || (!has_offsets && read_len < 0);
    return bad ? arg_invalid(name, "bad argument") : ArgCheck{};
}
inline ArgCheck check_update_host_args(const std::string &name, bool has_counter, bool has_offsets, int64_t n_reads)
{
    const bool bad = !has_counter || n_reads < 0 || (n_reads > 0 && !has_offsets);
    return bad ? arg_invalid(name, "bad argument") : ArgCheck{};
}
inline ArgCheck check_update_host_bytes(const std::string &name, int64_t n_bytes, bool has_bases)
{
    return n_bytes < 0 || (n_bytes > 0 && !has_bases) ? arg_invalid(name, "bad offsets") : ArgCheck{};
}

// Of the host form: offsets[0 .. n_reads] (or nullptr) start at no negative byte and never descend.
inline ArgCheck check_ascending_offsets(const std::string &name, const int64_t *offsets, int64_t n_reads)
{
    if (!offsets)
        return ArgCheck{};
    if (offsets[0] < 0)
        return arg_invalid(name, "negative offset");
    for (int64_t i = 0; i < n_reads; ++i)
        if (offsets[i + 1] < offsets[i])
            return arg_invalid(name, "offsets descend at read " + std::to_string(i));
    return ArgCheck{};
}

} // namespace covest
