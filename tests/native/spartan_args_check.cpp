// spartan_args_check.cpp -- the host side of csrc/spartan.hip (argument rules, overlap checks, the conversion of the bind
// coefficients) as a stand-alone host program for a sanitizer run; no device code is built and no kernel can be launched.  Built
// and run by the recipe in the header of pcs_args_check.cpp (tests/helpers.py run_host_program).
// Every call in the first part must come back with ZK_ERR_ARG before anything is written; the last ones pass the checks, convert
// their scalars on the host and then fail in the launch (ZK_ERR_HIP: no device, and the empty image holds no kernel).
#include <cstdio>
#include <cstdlib>
#include "../../zksnake_amd/csrc/spartan.hip"

namespace zkmi {
int dev_alloc_cached(void** p, size_t bytes) { *p = malloc(bytes ? bytes : 1); return *p ? ZK_OK : ZK_ERR_HIP; }
void dev_free_cached(void* p) { free(p); }
}  // namespace zkmi

static int g_errors = 0;
#define EXPECT(call, want)                                                                       \
    do {                                                                                         \
        int got_ = (call);                                                                       \
        if (got_ != (want)) { printf("  FAILED line %d: %s = %d\n", __LINE__, #call, got_); ++g_errors; } \
    } while (0)

// a merged CSR of 2^2 segments with 8 entries, one long segment with 2 items, a table x of 2^3 elements; nothing is ever
// dereferenced by a call that is refused
static const int LOG_SEG = 2, N_SEG = 4, LOG_X = 3, N_X = 8, NNZ = 8, N_LONG = 1, N_ITEMS = 2;
static uint64_t g_fr[4 * (N_X + NNZ + 3 * N_SEG + N_ITEMS + N_SEG)];
static uint32_t g_u32[(3 * N_SEG + 1) + NNZ + N_LONG + (3 * N_LONG + 1) + 2 * N_ITEMS];

struct Args {
    int log_seg = LOG_SEG;
    uint64_t n_entries = NNZ;
    const void *ptr = g_u32, *idx = g_u32 + 13, *val = g_fr + 4 * N_X;
    uint64_t n_long = N_LONG;
    const void *long_segs = g_u32 + 21, *item_ptr = g_u32 + 22;
    uint64_t n_items = N_ITEMS;
    const void* items = g_u32 + 26;
    void* partials = g_fr + 4 * (N_X + NNZ + 3 * N_SEG);
    int log_x = LOG_X;
    const void* x = g_fr;
    void *az = g_fr + 4 * (N_X + NNZ), *bz = g_fr + 4 * (N_X + NNZ + N_SEG), *cz = g_fr + 4 * (N_X + NNZ + 2 * N_SEG);
    void* out = g_fr + 4 * (N_X + NNZ + 3 * N_SEG + N_ITEMS);
};

static uint64_t g_coeff[12];

static int products(int curve, const Args& a) {
    return zk_r1cs_products_dev(curve, a.log_seg, a.n_entries, a.ptr, a.idx, a.val, a.n_long, a.long_segs, a.item_ptr, a.n_items, a.items, a.partials,
                                a.log_x, a.x, a.az, a.bz, a.cz, nullptr);
}
static int bind(int curve, const Args& a, const uint64_t* coeff = g_coeff) {
    return zk_r1cs_bind_dev(curve, a.log_seg, a.n_entries, a.ptr, a.idx, a.val, a.n_long, a.long_segs, a.item_ptr, a.n_items, a.items, a.partials,
                            a.log_x, a.x, coeff, a.out, nullptr);
}
// both entry points must refuse
#define REFUSED(curve, a)                      \
    do {                                       \
        EXPECT(products(curve, a), ZK_ERR_ARG); \
        EXPECT(bind(curve, a), ZK_ERR_ARG);     \
    } while (0)

int main() {
    static_assert(ZK_R1CS_MAX_LOG == 24 && ZK_R1CS_LONG_ROW == 64, "the limits this program walks up to");
    for (int i = 0; i < 12; ++i) g_coeff[i] = ~0ull - i;   // above r: reduced on entry
    const uint64_t eb = 32;
    for (int curve = 0; curve < 2; ++curve) {
        Args a;
        // a null pointer
        a = Args(); a.ptr = nullptr; REFUSED(curve, a);
        a = Args(); a.idx = nullptr; REFUSED(curve, a);
        a = Args(); a.val = nullptr; REFUSED(curve, a);
        a = Args(); a.x = nullptr; REFUSED(curve, a);
        a = Args(); a.az = nullptr; EXPECT(products(curve, a), ZK_ERR_ARG);
        a = Args(); a.bz = nullptr; EXPECT(products(curve, a), ZK_ERR_ARG);
        a = Args(); a.cz = nullptr; EXPECT(products(curve, a), ZK_ERR_ARG);
        a = Args(); a.out = nullptr; EXPECT(bind(curve, a), ZK_ERR_ARG);
        a = Args(); EXPECT(bind(curve, a, nullptr), ZK_ERR_ARG);
        // log_seg, log_x out of range
        for (int bad : {-1, ZK_R1CS_MAX_LOG + 1, 63, 64}) {
            a = Args(); a.log_seg = bad; REFUSED(curve, a);
            a = Args(); a.log_x = bad; REFUSED(curve, a);
        }
        a = Args(); a.n_entries = 1ull << 32; REFUSED(curve, a);
        // n_long / n_items inconsistent with each other, with the entries, with the segments or with their pointers
        a = Args(); a.n_long = 3; REFUSED(curve, a);                       // more long segments than items
        a = Args(); a.n_items = NNZ + 1; REFUSED(curve, a);                // more items than entries
        a = Args(); a.n_long = 0; REFUSED(curve, a);                       // items without a long segment
        a = Args(); a.n_long = N_SEG + 1; a.n_items = N_SEG + 1; REFUSED(curve, a);   // more long segments than segments
        a = Args(); a.n_entries = 0; REFUSED(curve, a);
        a = Args(); a.long_segs = nullptr; REFUSED(curve, a);
        a = Args(); a.item_ptr = nullptr; REFUSED(curve, a);
        a = Args(); a.items = nullptr; REFUSED(curve, a);
        a = Args(); a.partials = nullptr; REFUSED(curve, a);
        // an output overlaps an input: the same start, its last element over the first of the input, its first over the last
        a = Args(); a.az = (void*)a.x; a.out = (void*)a.x; REFUSED(curve, a);
        a = Args(); a.cz = (char*)a.partials - eb * (N_SEG - 1) + eb * N_ITEMS; a.out = a.cz; REFUSED(curve, a);   // over the scratch's end
        a = Args(); a.bz = (char*)a.x + eb * (N_X - 1); a.out = a.bz; REFUSED(curve, a);
        a = Args(); a.az = (void*)a.val; a.out = (void*)a.val; REFUSED(curve, a);
        a = Args(); a.bz = (char*)a.val + eb * (NNZ - 1); a.out = a.bz; REFUSED(curve, a);
        a = Args(); a.cz = (void*)a.ptr; a.out = (void*)a.ptr; REFUSED(curve, a);
        a = Args(); a.az = (char*)a.ptr + 4 * 3 * N_SEG; a.out = a.az; REFUSED(curve, a);   // the last word of ptr
        a = Args(); a.az = (void*)a.idx; a.out = (void*)a.idx; REFUSED(curve, a);
        a = Args(); a.bz = (void*)a.long_segs; a.out = (void*)a.long_segs; REFUSED(curve, a);
        a = Args(); a.cz = (void*)a.item_ptr; a.out = (void*)a.item_ptr; REFUSED(curve, a);
        a = Args(); a.az = (void*)a.items; a.out = (void*)a.items; REFUSED(curve, a);
        // two outputs overlap; the scratch overlaps an output or an input
        a = Args(); a.bz = a.az; EXPECT(products(curve, a), ZK_ERR_ARG);
        a = Args(); a.cz = (char*)a.az + eb * (N_SEG - 1); EXPECT(products(curve, a), ZK_ERR_ARG);
        a = Args(); a.cz = (char*)a.bz - eb * (N_SEG - 1); EXPECT(products(curve, a), ZK_ERR_ARG);
        a = Args(); a.partials = a.az; a.out = a.az; REFUSED(curve, a);
        a = Args(); a.partials = (char*)a.cz + eb * (N_SEG - 1); EXPECT(products(curve, a), ZK_ERR_ARG);
        a = Args(); a.partials = (char*)a.out - eb * (N_ITEMS - 1); EXPECT(bind(curve, a), ZK_ERR_ARG);
        a = Args(); a.partials = (void*)a.x; REFUSED(curve, a);
        a = Args(); a.partials = (char*)a.val + eb * (NNZ - 1); REFUSED(curve, a);
        // past the checks: the coefficients are converted on the host, then the launch fails
        a = Args(); EXPECT(products(curve, a), ZK_ERR_HIP); EXPECT(bind(curve, a), ZK_ERR_HIP);
        a = Args(); a.n_long = a.n_items = 0; a.long_segs = a.item_ptr = a.items = nullptr; a.partials = nullptr;
        EXPECT(products(curve, a), ZK_ERR_HIP); EXPECT(bind(curve, a), ZK_ERR_HIP);
        a = Args(); a.n_entries = a.n_long = a.n_items = 0; a.idx = a.val = nullptr;    // all sub-segments empty
        EXPECT(products(curve, a), ZK_ERR_HIP); EXPECT(bind(curve, a), ZK_ERR_HIP);
        a = Args(); a.log_seg = 0; a.log_x = 0; a.n_long = a.n_items = 0;                // one segment, one element
        EXPECT(products(curve, a), ZK_ERR_HIP); EXPECT(bind(curve, a), ZK_ERR_HIP);
        a = Args(); a.out = (char*)a.partials + eb * N_ITEMS;                            // adjacent, not overlapping
        EXPECT(bind(curve, a), ZK_ERR_HIP);
    }
    {
        Args a;
        EXPECT(products(2, a), ZK_ERR_ARG); EXPECT(bind(2, a), ZK_ERR_ARG);
        EXPECT(products(-1, a), ZK_ERR_ARG); EXPECT(bind(-1, a), ZK_ERR_ARG);
    }
    for (unsigned i = 0; i < sizeof(g_fr) / sizeof(g_fr[0]); ++i)
        if (g_fr[i]) { printf("  FAILED: a refused call wrote to its buffers\n"); ++g_errors; break; }
    for (unsigned i = 0; i < sizeof(g_u32) / sizeof(g_u32[0]); ++i)
        if (g_u32[i]) { printf("  FAILED: a refused call wrote to its index arrays\n"); ++g_errors; break; }
    if (g_errors) printf("spartan_args_check: %d FAILED\n", g_errors);
    else printf("spartan_args_check: all ok\n");
    return g_errors ? 1 : 0;
}
