// reads_args_check.cpp -- the host-side check of the argument checks the entry points over packed reads share
// (covest_amd/csrc/reads_args.h), compiled and run by tests/test_reads_args_cpu.py with the host
// compiler under -fsanitize=address,undefined.  No device: each check is walked at its boundary, and the status and the
// exact text of the message are asserted.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "reads_args.h"

using namespace covest;

static const int64_t kMax = std::numeric_limits<int64_t>::max();

static void expect(const ArgCheck &got, int status, const std::string &message, int line)
{
    if (got.status != status || got.message != message) {
        std::printf("FAILED %s:%d: status %d \"%s\", expected %d \"%s\"\n", __FILE__, line, got.status, got.message.c_str(), status,
                    message.c_str());
        std::exit(1);
    }
}
#define OK(call) expect(call, COVEST_OK, "", __LINE__)
#define INVALID(call, text) expect(call, COVEST_E_INVALID, std::string("who: ") + text, __LINE__)

static const char *kNegative = "n_reads and first_read must not be negative";
static const char *kReadLen = "without offsets read_len must not be negative";
static const char *kReach = "more reads than 64-bit offsets reach";
static const char *kOutOffsets = "reads of their own lengths need an array for the output offsets";

// first_read + n_reads at INT64_MAX; n_reads * read_len either side of 2^63
static void check_reach()
{
    OK(check_reads_reach("who", 0, 0, 0));
    OK(check_reads_reach("who", kMax, 0, 1));
    OK(check_reads_reach("who", 0, kMax, 1));
    OK(check_reads_reach("who", kMax - 7, 7, 1));  // the sum is INT64_MAX
    INVALID(check_reads_reach("who", kMax - 7, 8, 1), kReach);
    INVALID(check_reads_reach("who", kMax, 1, 0), kReach);
    INVALID(check_reads_reach("who", 1, kMax, 0), kReach);
    // 2^63 = 2^31 * 2^32: one read fewer, or one base fewer a read, is within reach
    const int64_t a = (int64_t)1 << 31, b = (int64_t)1 << 32;
    INVALID(check_reads_reach("who", 0, a, b), kReach);
    INVALID(check_reads_reach("who", 0, b, a), kReach);
    OK(check_reads_reach("who", 0, a - 1, b));
    OK(check_reads_reach("who", 0, a, b - 1));
    OK(check_reads_reach("who", 0, kMax / 7, 7));  // 7 divides 2^63 - 1
    INVALID(check_reads_reach("who", 0, kMax / 7 + 1, 7), kReach);
    OK(check_reads_reach("who", 0, 1, kMax));
    INVALID(check_reads_reach("who", 0, 2, kMax), kReach);
    OK(check_reads_reach("who", 0, kMax, 0));      // reads with offsets of their own: no product
}

// the order of the four checks, and null and non-null output offsets
static void check_args()
{
    OK(check_reads_args("who", false, 0, 0, 0, false));
    OK(check_reads_args("who", false, 8, 100, 5, false));
    OK(check_reads_args("who", true, 8, -1, 5, true));           // read_len is not looked at beside offsets
    OK(check_reads_args("who", true, kMax, kMax, 0, true));       // ... nor multiplied
    OK(check_reads_args("who", true, 0, 0, 0, false));            // no reads: no output offsets needed
    OK(check_reads_args("who", false, 8, 100, 0, true));
    INVALID(check_reads_args("who", true, 1, 0, 0, false), kOutOffsets);
    INVALID(check_reads_args("who", true, 8, 100, 0, false), kOutOffsets);
    INVALID(check_reads_args("who", false, -1, -1, kMax, false), kNegative);
    INVALID(check_reads_args("who", true, 8, 0, -1, false), kNegative);
    INVALID(check_reads_args("who", false, kMax, -1, kMax, false), kReadLen);
    INVALID(check_reads_args("who", true, 8, 0, kMax - 7, false), kReach); // before the output offsets
    OK(check_reads_args("who", true, 7, 0, kMax - 7, true));
    INVALID(check_reads_args("who", false, (int64_t)1 << 62, 2, 0, true), kReach);
    OK(check_reads_args("who", false, ((int64_t)1 << 62) - 1, 2, 0, true));
    OK(check_reads_args("who", false, (int64_t)1 << 62, 0, 0, true)); // empty reads: no product to overflow
}

// offsets equal, descending at the first read and at the last, a negative first offset
static void check_offsets()
{
    OK(check_ascending_offsets("who", nullptr, 5));
    const std::vector<int64_t> equal(6, 7), rising = {0, 3, 3, 10, 11, 11}, one = {-1};
    OK(check_ascending_offsets("who", equal.data(), 5));
    OK(check_ascending_offsets("who", rising.data(), 5));
    OK(check_ascending_offsets("who", rising.data(), 0));
    std::vector<int64_t> bad = rising;
    bad[1] = -1; // (after a first offset of 0: it descends, it is not "negative")
    INVALID(check_ascending_offsets("who", bad.data(), 5), "offsets descend at read 0");
    bad = rising;
    bad[5] = 10;
    INVALID(check_ascending_offsets("who", bad.data(), 5), "offsets descend at read 4");
    OK(check_ascending_offsets("who", bad.data(), 4)); // (the last offset is not looked at)
    bad = rising;
    bad[0] = -1;
    INVALID(check_ascending_offsets("who", bad.data(), 5), "negative offset");
    INVALID(check_ascending_offsets("who", one.data(), 0), "negative offset"); // offsets[0] alone, with no read
    bad = {kMax, kMax - 1};
    INVALID(check_ascending_offsets("who", bad.data(), 1), "offsets descend at read 0");
}

// The device forms over a counter's table: the sizes at 0 and either side of 2^32, and what the table must hold -- the
// wide keys win over the partitioned result, as they did in each form.
static void check_table_forms()
{
    static const char *kSizes = "negative size, or no offsets and no read_len below 2^32";
    static const char *kWide = "who: k must be at most 31 (keys of one word)";
    static const char *kBulk = "the counter holds a covest_kmer_count_reads_device result (its keys are not in the table); "
                               "covest_kmer_clear first";
    const int64_t two32 = (int64_t)1 << 32;
    OK(check_table_reads_sizes("who", false, 0, 0));
    OK(check_table_reads_sizes("who", false, kMax, two32 - 1));
    OK(check_table_reads_sizes("who", true, 0, -1));      // read_len is not looked at beside offsets
    OK(check_table_reads_sizes("who", true, kMax, two32));
    OK(check_table_reads_sizes("who", true, 5, kMax));
    INVALID(check_table_reads_sizes("who", false, 0, two32), kSizes);
    INVALID(check_table_reads_sizes("who", false, 5, kMax), kSizes);
    INVALID(check_table_reads_sizes("who", false, 0, -1), kSizes);
    INVALID(check_table_reads_sizes("who", false, -1, 0), kSizes);
    INVALID(check_table_reads_sizes("who", true, -1, 0), kSizes);  // no reads below none, with offsets too
    OK(check_table_holds_keys("who", 0, false));
    INVALID(check_table_holds_keys("who", 0, true), kBulk);
    for (const int wide : {2, 4, 8}) {
        expect(check_table_holds_keys("who", wide, false), COVEST_E_UNSUPPORTED, kWide, __LINE__);
        expect(check_table_holds_keys("who", wide, true), COVEST_E_UNSUPPORTED, kWide, __LINE__);
    }
}

// The eight forms that change a counter's table (abi_update.cpp): every flag and size of the device forms' and the host
// forms' first check on its own and at 0 | 1 reads, and the host forms' bytes either side of 0.
static void check_update_forms()
{
    static const char *kArgument = "bad argument", *kBytes = "bad offsets";
    //                                    counter bases offsets n_reads read_len
    OK(check_update_device_args("who", true, true, true, 1, 100));
    OK(check_update_device_args("who", true, true, false, kMax, 0));      // reads of no bases, no offsets
    OK(check_update_device_args("who", true, false, false, 0, 0));        // no reads: no bases needed
    OK(check_update_device_args("who", true, false, true, 0, -1));        // read_len is not looked at beside offsets
    OK(check_update_device_args("who", true, true, true, kMax, kMax));
    INVALID(check_update_device_args("who", false, true, true, 1, 100), kArgument);
    INVALID(check_update_device_args("who", false, false, false, 0, 0), kArgument);
    INVALID(check_update_device_args("who", true, true, true, -1, 100), kArgument);
    INVALID(check_update_device_args("who", true, false, true, 1, 100), kArgument);   // one read and no bases
    INVALID(check_update_device_args("who", true, true, false, 1, -1), kArgument);
    INVALID(check_update_device_args("who", true, false, false, 0, -1), kArgument);   // ... also with no reads
    //                                  counter offsets n_reads
    OK(check_update_host_args("who", true, true, 1));
    OK(check_update_host_args("who", true, false, 0));                    // no reads: no offsets needed
    OK(check_update_host_args("who", true, true, kMax));
    INVALID(check_update_host_args("who", false, true, 1), kArgument);
    INVALID(check_update_host_args("who", false, false, 0), kArgument);
    INVALID(check_update_host_args("who", true, true, -1), kArgument);
    INVALID(check_update_host_args("who", true, false, 1), kArgument);
    INVALID(check_update_host_args("who", true, false, -1), kArgument);
    //                                   n_bytes bases
    OK(check_update_host_bytes("who", 0, false));                         // reads that are all empty: no bases needed
    OK(check_update_host_bytes("who", 0, true));
    OK(check_update_host_bytes("who", 1, true));
    OK(check_update_host_bytes("who", kMax, true));
    INVALID(check_update_host_bytes("who", 1, false), kBytes);
    INVALID(check_update_host_bytes("who", -1, true), kBytes);            // offsets[n_reads] below offsets[0]
    INVALID(check_update_host_bytes("who", -1, false), kBytes);
    INVALID(check_update_host_bytes("who", -kMax - 1, true), kBytes);
}

int main()
{
    check_reach();
    check_args();
    check_offsets();
    check_table_forms();
    check_update_forms();
    // a name is taken as it comes
    expect(check_reads_reach("covest_sample_reads_device", kMax, 1, 0), COVEST_E_INVALID,
           "covest_sample_reads_device: more reads than 64-bit offsets reach", __LINE__);
    std::printf("reads_args ok\n");
    return 0;
}
