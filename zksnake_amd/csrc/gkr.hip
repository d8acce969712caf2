// gkr.hip -- the sparse side of the GKR prover and verifier for layered circuits over BN254 Fr / BLS12-381 Fr (gfx950).
//
// Stands in for what the reference does with dense selector polynomials of n_j + 2 n_(j-1) variables
// (python/zksnake/subprotocol/gkr.py:113-186): the wiring predicates add_j, mul_j have ONE non-zero entry per gate, so every
// sum over them here is a sum over gates (the bookkeeping of Libra, Xie et al. 2019), linear in the layer's size:
//   layer evaluation   W_j[g] = type_g ? W_(j-1)[b_g] W_(j-1)[c_g] : W_(j-1)[b_g] + W_(j-1)[c_g]
//   eq table           E[x] = prod_t (bit t of x ? r_t : 1 - r_t)
//   phase 1 (rows b)   P[b] = sum_ADD E[a] + sum_MUL E[a] W[c],     Q[b] = sum_ADD E[a] W[c]
//   phase 2 (rows c)   Aadd[c] = sum_ADD E[a] E2[b],                Amul[c] = sum_MUL E[a] E2[b]
//   wiring evaluation  add~(r,u,v), mul~(r,u,v) = sum over ADD (MUL) gates of E_r[a] E_u[b] E_v[c]
// A gate is (type u8: 0 ADD, 1 MUL; in1 u32; in2 u32); the host has checked in1, in2 < n_(j-1) when it compiled the circuit, so
// the gathers below never leave their tables.  The two phases read the gates through a static CSR (grouped by in1 for phase 1,
// by in2 for phase 2) whose rows are split by length as spmv_kernel's are (spmv.hip): one lane per short row; a row longer than
// GKR_LONG_ROW is cut on the host into work items, one workgroup sums each item and one workgroup then adds up each long row.
// Every row is written by exactly one thread, empty rows as zero: no atomics, and the outputs never need clearing.
//
// Like mle.hip the kernels multiply canonical data directly: mont(x, y) = x y / R, so a sum of single products is closed with
// R^2 and a sum of double products with R^3, once per thread, before the fixed-order workgroup sums of fr_sum.hip.h.
// Workgroups of MLE_TILE threads; the strided grids are capped at FR_MAX_BLOCKS (2^18 threads: item 2^18 is a second stride).
#include "fr_sum.hip.h"

namespace zkmi {

constexpr int GKR_MAX_LOG = ZK_GKR_MAX_LOG;
// the cap under the name tests/test_gpu_gkr.py reads from this file to place its sizes; the launches use FR_MAX_BLOCKS
constexpr unsigned GKR_MAX_BLOCKS = 1024;
static_assert(GKR_MAX_BLOCKS == FR_MAX_BLOCKS, "the sizes of tests/test_gpu_gkr.py sit on the shared cap");
constexpr uint32_t GKR_LONG_ROW = ZK_GKR_LONG_ROW;

// ---- layer evaluation ------------------------------------------------------------------------------------------------
// g < n_gates: the gate's value; n_gates <= g < n_out: zero (the padding of the dense table)
template <class P>
__global__ __launch_bounds__(MLE_TILE) void gkr_layer_eval_kernel(uint64_t n_gates, uint64_t n_out, const uint8_t* __restrict__ types,
                                                                  const uint32_t* __restrict__ in1, const uint32_t* __restrict__ in2,
                                                                  const uint32_t* __restrict__ w, uint32_t* __restrict__ out) {
    const uint64_t stride = (uint64_t)gridDim.x * MLE_TILE;
    const Fp<P> r2 = fp_const<P>(P::R2);
    for (uint64_t g = (uint64_t)blockIdx.x * MLE_TILE + threadIdx.x; g < n_out; g += stride) {
        Fp<P> v = fp_zero<P>();
        if (g < n_gates) {
            const Fp<P> x = load_fr<P>(w + (size_t)in1[g] * P::W), y = load_fr<P>(w + (size_t)in2[g] * P::W);
            v = types[g] ? fp_mul<P>(fp_mul<P>(x, y), r2) : fp_add<P>(x, y);
        }
        store_fr<P>(out + g * P::W, fp_reduce_full<P>(v));
    }
}

// ---- eq table --------------------------------------------------------------------------------------------------------
template <class P>
struct EqArgs {
    Fp<P> r_m[GKR_MAX_LOG], nr_m[GKR_MAX_LOG];  // r_t R and (1 - r_t) R
};

template <class P>
__global__ __launch_bounds__(MLE_TILE) void gkr_eq_table_kernel(uint64_t n, int k, EqArgs<P> a, uint32_t* __restrict__ out) {
    const uint64_t stride = (uint64_t)gridDim.x * MLE_TILE;
    for (uint64_t x = (uint64_t)blockIdx.x * MLE_TILE + threadIdx.x; x < n; x += stride) {
        Fp<P> v = fp_raw_one<P>();   // the integer 1: the start of a chain of products by Montgomery-form factors
        for (int t = 0; t < k; ++t) v = fp_mul<P>(v, (x >> t) & 1 ? a.r_m[t] : a.nr_m[t]);
        store_fr<P>(out + x * P::W, fp_reduce_full<P>(v));
    }
}

// ---- the two bookkeeping passes ----------------------------------------------------------------------------------------
// Entry e of the CSR is a gate: gate[e] = its index a in its own layer, other[e] = the input that is NOT the row (c in phase 1,
// b in phase 2), types[e].  One product per entry, t = E[a] Y[other] / R with Y = W (phase 1) or E2 (phase 2).
template <class P>
struct PhaseAcc {
    Fp<P> add_t, mul_t, add_e;   // sums of t over ADD gates, of t over MUL gates, and (phase 1) of E[a] itself over ADD gates
};

template <class P>
__device__ __forceinline__ Fp<P> fp_sel(bool c, const Fp<P>& a, const Fp<P>& b) {
    Fp<P> o;
#pragma unroll
    for (int l = 0; l < P::N; ++l) o.v[l] = c ? a.v[l] : b.v[l];
    return o;
}

template <class P, int PHASE>
__device__ __forceinline__ void phase_entry(PhaseAcc<P>& acc, uint32_t e, const uint32_t* __restrict__ gate, const uint32_t* __restrict__ other,
                                            const uint8_t* __restrict__ types, const uint32_t* __restrict__ tab_e, const uint32_t* __restrict__ tab_y) {
    const Fp<P> ea = load_fr<P>(tab_e + (size_t)gate[e] * P::W);
    const Fp<P> t = fp_mul<P>(ea, load_fr<P>(tab_y + (size_t)other[e] * P::W));
    // limb-wise selects, not a branch per type: a branch makes the compiler address the accumulators through memory (scratch)
    const bool mul = types[e] != 0;
    const Fp<P> sum = fp_add<P>(fp_sel<P>(mul, acc.mul_t, acc.add_t), t);
    acc.mul_t = fp_sel<P>(mul, sum, acc.mul_t);
    acc.add_t = fp_sel<P>(mul, acc.add_t, sum);
    if (PHASE == 1) acc.add_e = fp_add<P>(acc.add_e, fp_sel<P>(mul, fp_zero<P>(), ea));
}

// the thread's two outputs as true values: phase 1 (P, Q) = (add_e + mul_t R, add_t R), phase 2 (Aadd, Amul) = (add_t R, mul_t R)
template <class P, int PHASE>
__device__ __forceinline__ void phase_close(const PhaseAcc<P>& acc, Fp<P>& o0, Fp<P>& o1) {
    const Fp<P> r2 = fp_const<P>(P::R2);
    if (PHASE == 1) {
        o0 = fp_add<P>(acc.add_e, fp_mul<P>(acc.mul_t, r2));
        o1 = fp_mul<P>(acc.add_t, r2);
    } else {
        o0 = fp_mul<P>(acc.add_t, r2);
        o1 = fp_mul<P>(acc.mul_t, r2);
    }
}

template <class P>
__device__ __forceinline__ PhaseAcc<P> phase_acc_zero() {
    PhaseAcc<P> acc;
    acc.add_t = acc.mul_t = acc.add_e = fp_zero<P>();
    return acc;
}

// one lane per row of at most GKR_LONG_ROW entries (an empty row writes zeros); longer rows are left to the two kernels below
template <class P, int PHASE>
__global__ __launch_bounds__(MLE_TILE) void gkr_phase_rows_kernel(uint64_t n_rows, const uint32_t* __restrict__ row_ptr,
                                                                  const uint32_t* __restrict__ gate, const uint32_t* __restrict__ other,
                                                                  const uint8_t* __restrict__ types, const uint32_t* __restrict__ tab_e,
                                                                  const uint32_t* __restrict__ tab_y, uint32_t* __restrict__ out0,
                                                                  uint32_t* __restrict__ out1) {
    const uint64_t row = (uint64_t)blockIdx.x * MLE_TILE + threadIdx.x;
    if (row >= n_rows) return;
    const uint32_t e0 = row_ptr[row], e1 = row_ptr[row + 1];
    if (e1 - e0 > GKR_LONG_ROW) return;
    PhaseAcc<P> acc = phase_acc_zero<P>();
    for (uint32_t e = e0; e < e1; ++e) phase_entry<P, PHASE>(acc, e, gate, other, types, tab_e, tab_y);
    Fp<P> o0, o1;
    phase_close<P, PHASE>(acc, o0, o1);
    store_fr<P>(out0 + row * P::W, fp_reduce_full<P>(o0));
    store_fr<P>(out1 + row * P::W, fp_reduce_full<P>(o1));
}

// one workgroup per work item [e0, e1) of a long row: partials[2 item], partials[2 item + 1] = the item's share of the two outputs
template <class P, int PHASE>
__global__ __launch_bounds__(MLE_TILE) void gkr_phase_items_kernel(const uint32_t* __restrict__ items, const uint32_t* __restrict__ gate,
                                                                   const uint32_t* __restrict__ other, const uint8_t* __restrict__ types,
                                                                   const uint32_t* __restrict__ tab_e, const uint32_t* __restrict__ tab_y,
                                                                   uint32_t* __restrict__ partials) {
    __shared__ uint32_t lds[P::N][MLE_TILE];
    const uint32_t e0 = items[2 * blockIdx.x], e1 = items[2 * blockIdx.x + 1];
    PhaseAcc<P> acc = phase_acc_zero<P>();
    for (uint32_t e = e0 + threadIdx.x; e < e1; e += MLE_TILE) phase_entry<P, PHASE>(acc, e, gate, other, types, tab_e, tab_y);
    Fp<P> o0, o1;
    phase_close<P, PHASE>(acc, o0, o1);
    uint32_t* dst = partials + (size_t)blockIdx.x * 2 * P::W;
    block_sum_store<P>(o0, lds, dst);
    block_sum_store<P>(o1, lds, dst + P::W);
}

// one workgroup per long row adds up its items
template <class P>
__global__ __launch_bounds__(MLE_TILE) void gkr_phase_long_kernel(const uint32_t* __restrict__ long_rows, const uint32_t* __restrict__ item_ptr,
                                                                  const uint32_t* __restrict__ partials, uint32_t* __restrict__ out0,
                                                                  uint32_t* __restrict__ out1) {
    __shared__ uint32_t lds[P::N][MLE_TILE];
    const uint32_t i0 = item_ptr[blockIdx.x], i1 = item_ptr[blockIdx.x + 1];
    const size_t row = long_rows[blockIdx.x];
    Fp<P> o0 = fp_zero<P>(), o1 = o0;
    for (uint32_t i = i0 + threadIdx.x; i < i1; i += MLE_TILE) {
        o0 = fp_add<P>(o0, load_fr<P>(partials + (size_t)i * 2 * P::W));
        o1 = fp_add<P>(o1, load_fr<P>(partials + ((size_t)i * 2 + 1) * P::W));
    }
    block_sum_store<P>(o0, lds, out0 + row * P::W);
    block_sum_store<P>(o1, lds, out1 + row * P::W);
}

// ---- wiring predicates at a point ----------------------------------------------------------------------------------------
// partial[2 blk] = sum over the workgroup's ADD gates of E_r[g] E_u[in1] E_v[in2], partial[2 blk + 1] the same over its MUL gates
template <class P>
__global__ __launch_bounds__(MLE_TILE) void gkr_wiring_kernel(uint64_t n_gates, const uint8_t* __restrict__ types, const uint32_t* __restrict__ in1,
                                                              const uint32_t* __restrict__ in2, const uint32_t* __restrict__ er,
                                                              const uint32_t* __restrict__ eu, const uint32_t* __restrict__ ev,
                                                              uint32_t* __restrict__ partial) {
    __shared__ uint32_t lds[P::N][MLE_TILE];
    Fp<P> sa = fp_zero<P>(), sm = sa;
    const uint64_t stride = (uint64_t)gridDim.x * MLE_TILE;
    for (uint64_t g = (uint64_t)blockIdx.x * MLE_TILE + threadIdx.x; g < n_gates; g += stride) {
        const Fp<P> t = fp_mul<P>(fp_mul<P>(load_fr<P>(er + g * P::W), load_fr<P>(eu + (size_t)in1[g] * P::W)),
                                  load_fr<P>(ev + (size_t)in2[g] * P::W));
        if (types[g]) sm = fp_add<P>(sm, t);
        else sa = fp_add<P>(sa, t);
    }
    const Fp<P> r2 = fp_const<P>(P::R2);
    const Fp<P> r3 = fp_mul<P>(r2, r2);   // every term carries R^-2: closed once per thread
    uint32_t* dst = partial + (size_t)blockIdx.x * 2 * P::W;
    block_sum_store<P>(fp_mul<P>(sa, r3), lds, dst);
    block_sum_store<P>(fp_mul<P>(sm, r3), lds, dst + P::W);
}

// ---- host side -----------------------------------------------------------------------------------------------------

static bool gkr_log_ok(int log_n) { return log_n >= 0 && log_n <= GKR_MAX_LOG; }

template <class P>
static int gkr_layer_eval_impl(uint64_t n_gates, const void* types, const void* in1, const void* in2, int log_prev, const void* w, int log_out,
                               void* out, hipStream_t st) {
    if (!gkr_log_ok(log_prev) || !gkr_log_ok(log_out)) return fail(ZK_ERR_ARG, "gkr_layer_eval: a layer has at most 2^24 wires");
    if (n_gates > (1ull << log_out)) return fail(ZK_ERR_ARG, "gkr_layer_eval: more gates than the output table holds");
    if (!w || !out || (n_gates && (!types || !in1 || !in2))) return fail(ZK_ERR_ARG, "gkr_layer_eval: null argument");
    const uint64_t eb = P::W * 4, n_out = 1ull << log_out;
    if (ranges_overlap(out, eb << log_out, w, eb << log_prev)) return fail(ZK_ERR_ARG, "gkr_layer_eval: d_out overlaps d_w");
    if (n_gates && (ranges_overlap(out, eb << log_out, types, n_gates) || ranges_overlap(out, eb << log_out, in1, 4 * n_gates) ||
                    ranges_overlap(out, eb << log_out, in2, 4 * n_gates)))
        return fail(ZK_ERR_ARG, "gkr_layer_eval: d_out overlaps the gates");
    hipLaunchKernelGGL(gkr_layer_eval_kernel<P>, dim3(fr_blocks(n_out)), dim3(MLE_TILE), 0, st, n_gates, n_out, (const uint8_t*)types,
                       (const uint32_t*)in1, (const uint32_t*)in2, (const uint32_t*)w, (uint32_t*)out);
    ZK_HIP(hipGetLastError());
    return ZK_OK;
}

template <class P>
static int gkr_eq_table_impl(int k, const uint64_t* r, void* out, hipStream_t st) {
    if (!gkr_log_ok(k)) return fail(ZK_ERR_ARG, "gkr_eq_table: need 0 <= k <= 24");
    if (!out || (k && !r)) return fail(ZK_ERR_ARG, "gkr_eq_table: null argument");
    EqArgs<P> a;
    const Fp<P> one_m = fp_one<P>();
    for (int t = 0; t < GKR_MAX_LOG; ++t) {
        a.r_m[t] = a.nr_m[t] = fp_zero<P>();
        if (t < k) {
            a.r_m[t] = fr_mont<P>(r + 4 * t);
            a.nr_m[t] = fp_sub<P>(one_m, a.r_m[t]);
        }
    }
    const uint64_t n = 1ull << k;
    hipLaunchKernelGGL(gkr_eq_table_kernel<P>, dim3(fr_blocks(n)), dim3(MLE_TILE), 0, st, n, k, a, (uint32_t*)out);
    ZK_HIP(hipGetLastError());
    return ZK_OK;
}

struct GkrCsr {
    int log_rows;
    uint64_t n_entries;
    const void *row_ptr, *gate, *other, *types;
    uint64_t n_long, n_items;
    const void *long_rows, *item_ptr, *items;
    void* partials;
};

template <class P, int PHASE>
static int gkr_phase_impl(const GkrCsr& c, int log_e, const void* tab_e, const void* tab_y, void* out0, void* out1, hipStream_t st) {
    if (!gkr_log_ok(c.log_rows) || !gkr_log_ok(log_e)) return fail(ZK_ERR_ARG, "gkr_phase: a layer has at most 2^24 wires");
    if (c.n_entries > (1ull << log_e)) return fail(ZK_ERR_ARG, "gkr_phase: more gates than the layer's table holds");
    if (!c.row_ptr || !tab_e || !tab_y || !out0 || !out1 || (c.n_entries && (!c.gate || !c.other || !c.types)))
        return fail(ZK_ERR_ARG, "gkr_phase: null argument");
    if (c.n_long > c.n_items || c.n_items > c.n_entries) return fail(ZK_ERR_ARG, "gkr_phase: more long rows than items, or more items than gates");
    if (c.n_long && (!c.long_rows || !c.item_ptr || !c.items || !c.partials)) return fail(ZK_ERR_ARG, "gkr_phase: null long-row argument");
    const uint64_t eb = P::W * 4, n_rows = 1ull << c.log_rows;
    const void* ins[9] = {tab_e, tab_y, c.row_ptr, c.gate, c.other, c.types, c.long_rows, c.item_ptr, c.items};
    const uint64_t in_len[9] = {eb << log_e, eb << c.log_rows, 4 * (n_rows + 1), 4 * c.n_entries, 4 * c.n_entries, c.n_entries,
                                4 * c.n_long, 4 * (c.n_long + 1), 8 * c.n_items};
    void* outs[3] = {out0, out1, c.n_long ? c.partials : nullptr};
    const uint64_t out_len[3] = {eb * n_rows, eb * n_rows, 2 * eb * c.n_items};
    for (int x = 0; x < 3; ++x) {
        if (!outs[x]) continue;
        if (overlaps_any(outs[x], out_len[x], ins, in_len, 9)) return fail(ZK_ERR_ARG, "gkr_phase: an output overlaps an input");
        if (overlaps_any(outs[x], out_len[x], outs, out_len, x)) return fail(ZK_ERR_ARG, "gkr_phase: two outputs overlap");
    }
    hipLaunchKernelGGL((gkr_phase_rows_kernel<P, PHASE>), dim3((unsigned)((n_rows + MLE_TILE - 1) / MLE_TILE)), dim3(MLE_TILE), 0, st, n_rows,
                       (const uint32_t*)c.row_ptr, (const uint32_t*)c.gate, (const uint32_t*)c.other, (const uint8_t*)c.types,
                       (const uint32_t*)tab_e, (const uint32_t*)tab_y, (uint32_t*)out0, (uint32_t*)out1);
    if (c.n_long) {
        hipLaunchKernelGGL((gkr_phase_items_kernel<P, PHASE>), dim3((unsigned)c.n_items), dim3(MLE_TILE), 0, st, (const uint32_t*)c.items,
                           (const uint32_t*)c.gate, (const uint32_t*)c.other, (const uint8_t*)c.types, (const uint32_t*)tab_e,
                           (const uint32_t*)tab_y, (uint32_t*)c.partials);
        hipLaunchKernelGGL(gkr_phase_long_kernel<P>, dim3((unsigned)c.n_long), dim3(MLE_TILE), 0, st, (const uint32_t*)c.long_rows,
                           (const uint32_t*)c.item_ptr, (const uint32_t*)c.partials, (uint32_t*)out0, (uint32_t*)out1);
    }
    ZK_HIP(hipGetLastError());
    return ZK_OK;
}

template <class P>
static int gkr_wiring_eval_impl(uint64_t n_gates, const void* types, const void* in1, const void* in2, int log_a, const void* er, int log_prev,
                                const void* eu, const void* ev, uint64_t* out, hipStream_t st) {
    if (!gkr_log_ok(log_a) || !gkr_log_ok(log_prev)) return fail(ZK_ERR_ARG, "gkr_wiring_eval: a layer has at most 2^24 wires");
    if (n_gates > (1ull << log_a)) return fail(ZK_ERR_ARG, "gkr_wiring_eval: more gates than the layer's table holds");
    if (!er || !eu || !ev || !out || (n_gates && (!types || !in1 || !in2))) return fail(ZK_ERR_ARG, "gkr_wiring_eval: null argument");
    FrSum<P> sum;
    ZK_HIP_RC(sum.alloc(fr_blocks(n_gates), 2));   // no gate: one workgroup, which stores two zeros
    hipLaunchKernelGGL(gkr_wiring_kernel<P>, dim3(sum.blocks), dim3(MLE_TILE), 0, st, n_gates, (const uint8_t*)types, (const uint32_t*)in1,
                       (const uint32_t*)in2, (const uint32_t*)er, (const uint32_t*)eu, (const uint32_t*)ev, sum.part());
    return sum.finish(out, st);
}

}  // namespace zkmi

using namespace zkmi;

extern "C" {

int zk_gkr_layer_eval_dev(int curve, uint64_t n_gates, const void* d_types, const void* d_in1, const void* d_in2, int log_prev, const void* d_w,
                          int log_out, void* d_out, void* stream) {
#define CALL(P) return gkr_layer_eval_impl<P>(n_gates, d_types, d_in1, d_in2, log_prev, d_w, log_out, d_out, (hipStream_t)stream)
    ZK_DISPATCH_FR(curve, CALL);
#undef CALL
}

int zk_gkr_eq_table_dev(int curve, int k, const uint64_t* r, void* d_out, void* stream) {
#define CALL(P) return gkr_eq_table_impl<P>(k, r, d_out, (hipStream_t)stream)
    ZK_DISPATCH_FR(curve, CALL);
#undef CALL
}

#define GKR_CSR_ARGS                                                                                                                  \
    const GkrCsr csr = {log_rows, n_entries, d_row_ptr, d_gate, d_other, d_types, n_long, n_items, d_long_rows, d_item_ptr, d_items, \
                        d_partials}

int zk_gkr_phase1_dev(int curve, int log_rows, uint64_t n_entries, const void* d_row_ptr, const void* d_gate, const void* d_other,
                      const void* d_types, uint64_t n_long, const void* d_long_rows, const void* d_item_ptr, uint64_t n_items,
                      const void* d_items, void* d_partials, int log_e, const void* d_e, const void* d_w, void* d_p, void* d_q, void* stream) {
    GKR_CSR_ARGS;
#define CALL(P) return gkr_phase_impl<P, 1>(csr, log_e, d_e, d_w, d_p, d_q, (hipStream_t)stream)
    ZK_DISPATCH_FR(curve, CALL);
#undef CALL
}

int zk_gkr_phase2_dev(int curve, int log_rows, uint64_t n_entries, const void* d_row_ptr, const void* d_gate, const void* d_other,
                      const void* d_types, uint64_t n_long, const void* d_long_rows, const void* d_item_ptr, uint64_t n_items,
                      const void* d_items, void* d_partials, int log_e, const void* d_e, const void* d_e2, void* d_add, void* d_mul,
                      void* stream) {
    GKR_CSR_ARGS;
#define CALL(P) return gkr_phase_impl<P, 2>(csr, log_e, d_e, d_e2, d_add, d_mul, (hipStream_t)stream)
    ZK_DISPATCH_FR(curve, CALL);
#undef CALL
}
#undef GKR_CSR_ARGS

int zk_gkr_wiring_eval_dev(int curve, uint64_t n_gates, const void* d_types, const void* d_in1, const void* d_in2, int log_a, const void* d_er,
                           int log_prev, const void* d_eu, const void* d_ev, uint64_t* out, void* stream) {
#define CALL(P) return gkr_wiring_eval_impl<P>(n_gates, d_types, d_in1, d_in2, log_a, d_er, log_prev, d_eu, d_ev, out, (hipStream_t)stream)
    ZK_DISPATCH_FR(curve, CALL);
#undef CALL
}

}  // extern "C"
