/*
 * zkmi.h -- C ABI of libzkmi.so, the MI355X (gfx950) proving backend that replaces the
 * field/curve hot path of Merricx/zksnake behind Groth16.prove()/Plonk.prove().
 *
 * Drop-in boundary: the reference crosses from Python into Rust through the pyo3 module
 * `zksnake._algebra` (reference src/lib.rs:6-185).  Each entry point below names the pyo3
 * function(s) it stands in for (file:line under the reference tree).  INTEGRATION.md shows the
 * ctypes stub a maintainer would add to python/zksnake/{ecc,polynomial}.py.
 *
 * Conventions (all entry points):
 *   - plain pointers and sizes only; no C++/torch types; never throws; returns an int status;
 *     zk_last_error() gives the message of the last failure on the calling thread.
 *   - field elements: canonical (non-Montgomery) integers as little-endian 64-bit limbs.
 *       Fr (both curves): 4 limbs.  Fq: 4 limbs (BN254) / 6 limbs (BLS12-381).
 *     Values >= modulus are reduced on entry, like `Fr::from(BigUint)` in the reference
 *     (src/bn254/polynomial.rs:538, src/bn254/curve.rs:359).
 *   - points: affine (x, y); G1 = 2 Fq elements, G2 = 4 (x.c0, x.c1, y.c0, y.c1); the point at
 *     infinity is the all-zero encoding ((0,0) is on none of the four curves since b != 0).
 *   - "host" functions take host memory and copy; "_dev" functions take HIP device pointers
 *     (e.g. torch tensor data_ptr()) plus a hipStream_t passed as void* (NULL = default stream).
 *   - the caller owns every buffer it passes; handles are freed explicitly.
 *   - calls may come from several threads (ctypes releases the GIL): the library serialises GPU
 *     work per handle internally.
 */
#ifndef ZKMI_H
#define ZKMI_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ZK_CURVE_BN254 0
#define ZK_CURVE_BLS12_381 1
#define ZK_G1 1
#define ZK_G2 2

#define ZK_OK 0
#define ZK_ERR_LENGTH 1        /* "Number of points and scalars mismatch" (src/bn254/curve.rs:369-371) */
#define ZK_ERR_DOMAIN 2        /* domain larger than 2^two-adicity (polynomial.rs:48 unwrap / :638 error) */
#define ZK_ERR_HIP 3           /* HIP / RCCL runtime failure, or no GPU present */
#define ZK_ERR_POINT 4         /* bad point encoding / not on curve (curve.rs:137-140) */
#define ZK_ERR_ARG 5           /* invalid curve/group/size argument */
#define ZK_ERR_NOT_DIVISIBLE 6 /* (U*V - W) mod Z != 0 (groth16/qap.py:67-69) */

/* ---- lifecycle ------------------------------------------------------------------------- */

int zk_init(int device);            /* select the HIP device for this process; ZK_ERR_HIP when no GPU */

/* Hardware queues.  A proof keeps seven HIP streams busy; the HIP runtime maps streams onto GPU_MAX_HW_QUEUES hardware
 * queues (4 by default) and streams that share a queue run one after the other (~ +1 ms per Groth16 proof at 2^20).  The
 * variable is read once, when the HIP runtime starts (the process's first HIP call).  zk_init / zk_init_ex /
 * zk_hw_queues_prepare therefore set GPU_MAX_HW_QUEUES=12 BEFORE the library's first HIP call when the caller has not set
 * it and the runtime is not running yet (the reference has nothing like it: its prover is single-threaded CPU code behind
 * the GIL, src/lib.rs:6-185).  The status says what happened:
 *   ZK_QUEUES_SET_BY_LIBRARY  the library put the setting in place in time;
 *   ZK_QUEUES_CALLER          GPU_MAX_HW_QUEUES was already in the environment and was left alone (*queues = its value);
 *   ZK_QUEUES_TOO_LATE        the runtime was already running without the setting (e.g. torch touched the GPU before the
 *                             first zk_ call): results are unaffected, concurrent streams may serialise.  Call
 *                             zk_hw_queues_prepare() (no HIP call inside) right after loading the library, or export the
 *                             variable yourself, to avoid it.
 * The decision is taken once per process; later calls return the same status. */
#define ZK_QUEUES_SET_BY_LIBRARY 0
#define ZK_QUEUES_CALLER 1
#define ZK_QUEUES_TOO_LATE 2
int zk_hw_queues_prepare(int* queues /* may be NULL; 0 = runtime default */);
int zk_init_ex(int device, int* queue_status, int* queues);   /* zk_init + the status above (either pointer may be NULL) */
/* test aid: one wave that spins for `microseconds` on `stream` (used to observe whether streams overlap) */
int zk_debug_spin_dev(void* stream, uint64_t microseconds);
/* Free what the library caches: twiddle and QAP tables, per-stream scratch and events, every MSM plan and fixed-base table, the
 * block cache and the pooled streams.  The caller must have no call in flight.  Afterwards: MSM plan handles from before are
 * refused with ZK_ERR_ARG (handle values are never reused), events of zk_qap_h_dev_begin are invalid, buffers of zk_dev_alloc /
 * zk_host_alloc and streams of zk_stream_create still belong to the caller and stay valid, and every entry point rebuilds what it
 * needs on its next call.  Calling it again is a no-op. */
int zk_shutdown(void);
int zk_device_count(void);          /* number of visible HIP devices (0 without a GPU; never fails) */
const char* zk_last_error(void);
const char* zk_version(void);

/* raw device memory for bindings that do not bring their own allocator (hipMalloc/hipFree/hipMemcpy);
 * a torch tensor's data_ptr() is equally valid wherever a device pointer is expected. */
int zk_dev_alloc(uint64_t bytes, void** d_ptr);
int zk_dev_free(void* d_ptr);
int zk_dev_upload(void* d_dst, const void* h_src, uint64_t bytes);
int zk_dev_download(void* h_dst, const void* d_src, uint64_t bytes);
/* upload ordered on `stream` and asynchronous to the host when h_src is page-locked (zk_host_alloc): lets a host that
 * marshals a long witness chunk by chunk ship chunk k while it converts chunk k + 1 */
int zk_dev_upload_async(void* d_dst, const void* h_src, uint64_t bytes, void* stream);
int zk_dev_memset(void* d_dst, int value, uint64_t bytes);
/* the same, ordered on `stream` (NULL = default stream): zk_dev_memset runs on the legacy default stream, which does not
 * synchronise with the non-blocking streams of zk_stream_create */
int zk_dev_memset_async(void* d_dst, int value, uint64_t bytes, void* stream);
int zk_dev_synchronize(void);
/* page-locked host memory: a witness marshalled into it (and results copied out of it) moves at the link rate instead of
 * through the runtime's staging copies (32 MB of witness: ~0.6 ms against 2-3 ms from pageable memory) */
int zk_host_alloc(uint64_t bytes, void** h_ptr);
int zk_host_free(void* h_ptr);
/* HIP streams for callers that keep several device-resident pipelines in flight (the Python host has no HIP binding
 * of its own): non-blocking with respect to the default stream; high_priority != 0 asks for the top priority level. */
int zk_stream_create(int high_priority, void** stream);
/* Waits for the work queued on the stream, releases what the library keeps under its handle (the transform scratch vectors,
 * the event of zk_qap_h_dev_begin / zk_qap_uv_dev: an event handed out for this stream is invalid afterwards) and destroys
 * it.  NULL is a no-op. */
int zk_stream_destroy(void* stream);
int zk_stream_synchronize(void* stream);

/* limb counts, so bindings do not hard-code them */
int zk_fq_limbs(int curve);         /* 64-bit limbs per base-field element: 4 / 6 */
int zk_point_limbs(int curve, int group); /* 64-bit limbs per affine point */

/* ---- scalar-field vectors (polynomial_bn254 / polynomial_bls12_381 submodules) ----------
 * csrc/ntt.hip: the transforms and the QAP chain (zk_ntt*, zk_qap_*); csrc/frvec.hip: the element-wise operations
 * (zk_vec_*, zk_poly_div_vanishing); csrc/spmv.hip: the sparse products (zk_spmv_*). */

/* fft / ifft / coset_fft / coset_ifft (src/bn254/polynomial.rs:535-585).
 * `in` holds n_in elements; the domain is next_pow2(size); the input is zero-padded, or, when
 * longer than the domain, truncated to it (ark-poly 0.4.2 fft_in_place/ifft_in_place resize the
 * vector to the domain size; the crate is not vendored: parity unpinned); `out` receives the whole
 * domain in natural order. coset != 0 uses the reference's offset (= the domain generator). */
int zk_ntt(int curve, int inverse, int coset, uint64_t n_in, const uint64_t* in, uint64_t size, uint64_t* out);

/* mul_over_evaluation_domain / add_over_evaluation_domain (polynomial.rs:587-634): element-wise
 * over `size` entries; entries beyond n_a / n_b count as zero.  op: 0 = mul, 1 = add, 2 = sub.
 * Deliberate divergence at THIS level: the reference's add_over_evaluation_domain indexes a[i], b[i] for every i < size
 * and panics on a shorter input (polynomial.rs:594-597), while mul zero-pads (polynomial.rs:617-625); the C entry point zero-pads for
 * every op (one kernel, and the PlonK prover adds vectors of unequal length).  The drop-in Python layer restores the
 * reference's behaviour: `add_over_evaluation_domain` raises IndexError for a short input before it gets here
 * (zksnake_amd/_algebra.py). */
int zk_vec_op(int curve, int op, uint64_t size, uint64_t n_a, const uint64_t* a, uint64_t n_b, const uint64_t* b,
              uint64_t* out);

/* Polynomial.divide_by_vanishing_poly (polynomial.rs:466-489): coeffs (len) = q*(X^n - 1) + rem.
 * q must hold max(len - n, 0) elements, rem min(len, n). *rem_is_zero tells whether rem == 0. */
int zk_poly_div_vanishing(int curve, uint64_t n, uint64_t len, const uint64_t* coeffs, uint64_t* q, uint64_t* rem,
                          int* rem_is_zero);

/* Device-resident forms: in place on a vector of 2^log_n canonical Fr elements. */
int zk_ntt_dev(int curve, int inverse, int log_n, void* d_data, void* stream);
int zk_vec_op_dev(int curve, int op, uint64_t n, const void* d_a, const void* d_b, void* d_out, void* stream);
/* reduce every element below the modulus in place (Fr::from(BigUint), src/bn254/curve.rs:358-361): limb-array
 * witnesses handed to the device-resident provers are only ASSUMED canonical by the kernels behind them. */
int zk_vec_canon_dev(int curve, uint64_t n, void* d_x, void* stream);
/* d_out[k] = g^k for k < n, canonical (the powers of tau of a setup, python/zksnake/groth16/protocol.py:48-55) */
int zk_vec_powers_dev(int curve, uint64_t n, const uint64_t* g, void* d_out, void* stream);

/* SparseArray.dot (python/zksnake/array.py:36-44) as a CSR product over Fr on device-resident arrays:
 * row_ptr u32[n_rows + 1], cols u32[nnz], vals canonical Fr[nnz], w canonical Fr[n_cols] (cols must be < n_cols: the
 * host validates, SparseArray.to_csr), out canonical Fr[n_rows].  One lane per row; rows with more than
 * skip_longer_than entries (0 = never) are left untouched for zk_spmv_long_dev. */
int zk_spmv_dev(int curve, uint64_t n_rows, const void* d_row_ptr, const void* d_cols, const void* d_vals,
                const void* d_w, void* d_out, uint32_t skip_longer_than, void* stream);
/* The long rows of the same product: long_rows u32[n_long] (row indices), item_ptr u32[n_long + 1] into
 * items, items u32[n_items][2] = entry ranges [k0, k1) of at most a few thousand entries each (the host cuts the rows
 * once per matrix), partials = scratch of n_items Fr elements.  One workgroup per item, then one per long row. */
int zk_spmv_long_dev(int curve, uint64_t n_long, const void* d_long_rows, const void* d_item_ptr, uint64_t n_items,
                     const void* d_items, const void* d_cols, const void* d_vals, const void* d_w, void* d_partials,
                     void* d_out, void* stream);

/* Fused QAP.evaluate_witness tail (python/zksnake/groth16/qap.py:57-69): from the evaluation vectors
 * a = A.w, b = B.w, c = C.w (2^log_n canonical Fr elements each, device memory) compute in place the
 * coefficient vectors u = iNTT(a), v = iNTT(b) and write h (2^log_n elements, h[2^log_n - 1] = 0) with
 * u*v - w = h*(X^n - 1).  Everything stays in HBM.  With u v = P_lo + X^n P_hi the quotient is h = P_hi, and on the coset g*H of the
 * 2n-th root of unity g (g^n = -1) the values of u v interpolate P_lo - P_hi, so h = (w - d) / 2 with d = that interpolant: 3 iNTT(n)
 * + 2 NTT(n) of g^i-scaled coefficients + 1 iNTT(n), the scalings and the point-wise product folded into the transforms' passes
 * (the reference goes through the doubled domain: 2 NTT(2n) + iNTT(2n) + fold; same h).  log_n + 1 must not exceed the field's
 * two-adicity and log_n must not be negative (ZK_ERR_DOMAIN).  log_n = 0 is one point: u = a, v = b, h[0] = 0, and the
 * divisibility flag says whether a_0 b_0 == c_0.
 * d_work must hold 4 * 2^log_n elements.  *divisible (host int) is set to 0 when a_i b_i != c_i for some i, i.e. when
 * the division would leave a remainder (the reference raises ValueError there); h is meaningless in that case. */
int zk_qap_h_dev(int curve, int log_n, void* d_a_u, void* d_b_v, const void* d_c, void* d_h, void* d_work,
                 int* divisible, void* stream);
/* The same in two steps.  _begin puts the whole chain on the stream and returns; *uv_ready (may be NULL) receives an event,
 * owned by the library and reused by the next _begin on that stream, that fires once u and v are final (a third of the
 * way into the chain): MSMs over u and v can sort beside the rest of it (zk_msm_plan_wait_event).  _end copies the
 * divisibility flag back and synchronises the stream. */
int zk_qap_h_dev_begin(int curve, int log_n, void* d_a_u, void* d_b_v, const void* d_c, void* d_h, void* d_work, void* stream,
                       void** uv_ready);
int zk_qap_h_dev_end(int curve, int log_n, const void* d_work, int* divisible, void* stream);
/* Only the first third of the chain: u = iNTT(a) and / or v = iNTT(b) in place (either pointer may be NULL), enqueued on the
 * stream, with the same "u and v are final" event.  For a rank of a task-partitioned prover whose MSM reads u or v only
 * (python/zksnake/groth16/protocol.py:133-147: <tau_1, u>, <tau_1, v> and <tau_2, v> do not need h); no divisibility check --
 * the rank(s) holding <target_1, h> run the whole chain and report it. */
int zk_qap_uv_dev(int curve, int log_n, void* d_a_u, void* d_b_v, void* stream, void** uv_ready);

/* ---- curve groups (ec_bn254 / ec_bls12_381 submodules) ---------------------------------- */

/* multiscalar_mul_g1 / multiscalar_mul_g2 (src/bn254/curve.rs:356-392, bls12_381 :366-402):
 * out = sum_i scalars[i] * bases[i].  n_scalars != n_points -> ZK_ERR_LENGTH. */
int zk_msm(int curve, int group, uint64_t n_points, uint64_t n_scalars, const uint64_t* scalars,
           const uint64_t* bases, uint64_t* out);
/* zk_msm is the reference's call shape and pays for it on every call: the bases go to the device and into Montgomery form, a
 * workspace is built and torn down (2^20 BN254 G1 pairs: ~3.6 ms, of which the MSM itself is 1.5).  The library does NOT cache
 * bases behind this entry point: recognising "the same array" by pointer and a hash of sampled rows would return a wrong point
 * after an in-place change the samples miss, and hashing all 64 MB costs more than the MSM.  A caller that multiplies against the
 * same points more than once (a proving key) creates a plan once -- zk_msm_plan_create below -- and calls zk_msm_plan_run; the
 * Python layer does exactly that behind EllipticCurve.multiexp when it is handed a PointArray (zksnake_amd/_algebra.py). */

/* batch_multi_scalar_g1 / _g2 (src/bn254/curve.rs:326-354): out[i] = scalars[i] * bases[i];
 * broadcast != 0 means `bases` holds one point used for every scalar (ecc.py:93-94). */
int zk_batch_mul(int curve, int group, uint64_t n, const uint64_t* scalars, const uint64_t* bases, int broadcast,
                 uint64_t* out);

/* Device-resident bases ("proving key stays in HBM").  zk_msm_plan_create uploads/normalises the
 * bases once (host or device pointer per `bases_on_device`) and sizes the workspace for up to n
 * points.  flags: bit0 = precompute the per-window multiples 2^(c*w) * P_i so that every window
 * shares one bucket set (uses n * windows * point bytes of HBM); window_bits 0 = automatic. */
#define ZK_MSM_PRECOMPUTE 1
#define ZK_MSM_HIGH_PRIORITY 2 /* the plan's own stream (ZK_STREAM_PLAN) gets the top stream priority */
/* General (not ZK_MSM_PRECOMPUTE) plans of up to 2^22 points split every scalar with the group's endomorphism,
 * k = k1 + lambda k2 with |k1|, |k2| < 2^127, and run over the 2n points (P_i, phi(P_i)) -- phi = (beta x, y) on G1, the squared
 * untwist-Frobenius-twist map (c x, -y) on G2: the same number of bucket additions in half the windows, so half the bucket
 * sets to reduce and half the doublings in the tail.  The result is the same point.  This flag (or ZKMI_NO_GLV=1 in the
 * environment) keeps the plain 254/255-bit windows.  Two split-scalar plans share a sort (zk_msm_plan_enqueue_shared) only
 * within one group: G1 and G2 split against different eigenvalues. */
#define ZK_MSM_NO_GLV 4
int zk_msm_plan_create(int curve, int group, uint64_t n, const void* bases, int bases_on_device, int flags,
                       int window_bits, uint64_t* handle);
/* The same for a rank of a window-sharded MSM that will only ever run the windows
 * [window_first, window_first + window_count) (window_count 0 = all): the fixed-base table and the
 * workspace are sized for that range only -- 1/8 of the memory and of the table build on 8 ranks.
 * Runs outside the range fail with ZK_ERR_ARG.  Call zk_msm_plan_windows on a throw-away
 * n = 1 plan (or compute ceil((bits + 1) / c)) to learn the window count first. */
int zk_msm_plan_create_range(int curve, int group, uint64_t n, const void* bases, int bases_on_device, int flags,
                             int window_bits, int window_first, int window_count, uint64_t* handle);
/* A second plan over the SAME device-resident bases (and fixed-base table; shared, freed with the last user) with its
 * own workspace and stream, so that two MSMs against one key can be in flight together. */
int zk_msm_plan_clone(uint64_t handle, uint64_t* clone_handle);
int zk_msm_plan_destroy(uint64_t handle);
/* scalars: n_scalars <= plan n canonical Fr elements (host or device per `scalars_on_device`); the
 * first n_scalars bases are used (ecc.py:118-119 truncation rule).  Result: one affine point in host
 * memory.  window_first/window_count select a window range for multi-GPU sharding (count 0 = all):
 * the partial result then is sum over those windows of 2^(c*w) * W_w, so partials of disjoint ranges
 * add up to the full MSM. */
int zk_msm_plan_run(uint64_t handle, uint64_t n_scalars, const void* scalars, int scalars_on_device,
                    int window_first, int window_count, uint64_t* out, void* stream);
/* Asynchronous form: enqueue puts all GPU stages and the D2H copy of the per-window results on the
 * stream and returns; finish waits and runs the host tail.  One run may be in flight per plan.
 * ZK_STREAM_PLAN selects a stream owned by the plan, so several plans (the five MSMs of a Groth16 proof)
 * overlap: their latency-bound reduction stages hide behind other plans' accumulation kernels.  Plan streams
 * are ordinary blocking streams: they are ordered after earlier work on the NULL stream. */
#define ZK_STREAM_PLAN ((void*)(intptr_t)-1)
int zk_msm_plan_enqueue(uint64_t handle, uint64_t n_scalars, const void* scalars, int scalars_on_device,
                        int window_first, int window_count, void* stream);
/* zk_msm_plan_enqueue in two steps, for a caller that keeps several plans in flight and wants their accumulate kernels one
 * after the other: _sort puts the digits and the sort on the stream, _rest the accumulate kernel -- not before the
 * accumulate kernel of `after_handle`'s run has finished (0 = no such condition; that run's _rest / enqueue_shared must
 * have been issued already) -- then the reduction and the D2H copy.  A resident accumulate grid holds every wave slot of
 * the chip until it ends, so accumulate kernels that run side by side only delay each other's reductions, and the sorts
 * of plans enqueued later starve behind them; ordered, the sorts run first and every reduction but the last overlaps the
 * next plan's accumulate kernel.  zk_msm_plan_finish as usual. */
int zk_msm_plan_enqueue_sort(uint64_t handle, uint64_t n_scalars, const void* scalars, int scalars_on_device,
                             int window_first, int window_count, void* stream);
int zk_msm_plan_enqueue_rest(uint64_t handle, uint64_t after_handle);
/* the plan's own stream (ZK_STREAM_PLAN) waits for an event of another stream (e.g. zk_qap_h_dev_begin's uv_ready) before
 * whatever is enqueued on it next */
int zk_msm_plan_wait_event(uint64_t handle, void* event);
/* forget a run in flight (sorted only, or complete) without collecting its result: waits for the plan's stream */
int zk_msm_plan_cancel(uint64_t handle);
/* The same scalars against a second set of bases (Groth16: <tau_1, v> in G1 and <tau_2, v> in G2): run `handle` on the
 * digits and the sorted entry list of `lender_handle`'s run in flight instead of sorting again.  Both plans must have the
 * same size, window layout, mode and window range (else ZK_ERR_ARG: enqueue normally); finish both as usual.  A general-mode
 * G1 lender must have been created with ZK_MSM_NO_GLV (a split-scalar sort is of no use to a G2 plan). */
int zk_msm_plan_enqueue_shared(uint64_t handle, uint64_t lender_handle, void* stream);
int zk_msm_plan_finish(uint64_t handle, uint64_t* out);
int zk_msm_plan_windows(uint64_t handle, int* window_bits, int* n_windows);
/* the window width and count a plan over n points will use (window_bits 0 = automatic), without creating one: what a
 * rank needs to pick its share before zk_msm_plan_create_range */
int zk_msm_window_layout(int curve, int group, uint64_t n, int flags, int window_bits, int* window_bits_out, int* n_windows);
/* the same with the choice between the two layouts: all_windows != 0 is what zk_msm_plan_create takes (fixed-base plans of 2^20
 * points or more: 13 windows of 20 bits), 0 what zk_msm_plan_create_range takes (16 windows of 16 bits, which split evenly).  A rank
 * of a task-partitioned prover that holds an MSM whole uses the former. */
int zk_msm_window_layout_ex(int curve, int group, uint64_t n, int flags, int window_bits, int all_windows, int* window_bits_out,
                            int* n_windows);
/* entries one window of the plan sorts and accumulates: n, or 2n when the plan runs on endomorphism pairs */
int zk_msm_plan_entries(uint64_t handle, uint64_t* entries_per_window);
/* milliseconds of the stages of the last zk_msm_plan_run on this plan, measured with HIP events on
 * the launch stream(s): [0] digits+sort, [1] bucket accumulation (dominant kernel; summed over its launches),
 * [2] bucket combination + reduction + D2H, [3] host tail, [4] total.  Returns the number of floats written. */
int zk_msm_plan_timings(uint64_t handle, float* ms, int cap);
/* Tuning options of one plan (not in the reference: ark's MSM has no knobs).  Defaults come from the ZKMI_* environment
 * variables read when the plan is created; the run-time ones can be changed between runs of a live plan:
 *   "segment_lanes"     lanes the accumulate kernel aims at (<= the value at creation, >= 64)        ZKMI_SEG_LANES
 *   "sum_one_step"      1 = row / column sums of the bucket reduction in one launch                 ZKMI_SUM_ONE_STEP
 *   "lanes_per_output"  lanes per row / column sum of the one-step form (0 = automatic, 2 .. 64)    ZKMI_LPO
 *   "two_level_sort"    0 = one-level / bucket-range sorts only (windows <= 16 bits)                ZKMI_NO_TWO_LEVEL
 *   "priority_steps"    0 = the waves of the accumulate kernel keep one issue priority throughout   ZKMI_NO_PRIO_STEPS
 *                       (default 1: they step it down near the end of their segment, which keeps the waves of a SIMD together
 *                       when the kernel has the chip to itself; applies to zk_msm_plan_run / zk_msm_plan_enqueue only)
 *   "split_pairs"       Fp2 groups: 1 = the accumulate kernel gives a segment to a lane PAIR and splits every   ZKMI_SPLIT_PAIRS
 *                       Fp2 value by component over it (half the registers per lane), 0 = one lane per segment,
 *                       -1 = the group's default (BLS12-381 G2: on, BN254 G2: off; measured, msm_accumulate.hip.h)
 * Results never depend on them.  ZK_ERR_ARG for unknown names (including the creation-time options ZKMI_SORT_WGS,
 * ZKMI_FINE_LOG, ZKMI_NO_GLV, ZKMI_PRE_C), for values the plan cannot honour and while a run is in flight. */
int zk_msm_plan_set_option(uint64_t handle, const char* name, int64_t value);
/* Test aid: a read-only view of the plan's last run -- the device buffers every stage before the bucket reduction left behind
 * (read them with zk_dev_download; they stay valid and unchanged until the plan's next run or its destruction) and the scalars
 * that say how to read them.  `out` receives ZK_MSM_VIEW_SLOTS values; ZK_ERR_ARG when cap is smaller or while a run is in
 * flight (between zk_msm_plan_enqueue* and zk_msm_plan_finish).  With n_keys = groups * B, m = entries per window of the run:
 *   [0]  d_dig       digits, pw_count rows of `dstride` values from the plan's FIRST window on, uint16 (uint32 when wide);
 *                    value = signed digit + 2^(c-1); a split-scalar plan stores k1's digit of scalar i at 2i, k2's at 2i + 1
 *   [1]  d_bases     affine rows in Montgomery form: P_i; (P_i, phi(P_i)) at rows 2i, 2i + 1 of a split-scalar plan;
 *                    2^(c (pw_first + k)) P_i at row k n + i of a fixed-base plan
 *   [2]  sorted      bstart[n_keys] entry words (sign << 31 | row of d_bases), grouped by key = set * B + |digit| - 1
 *   [3]  bstart      n_keys + 1 offsets into sorted         [4]  sstart   n_keys + 1 run offsets (runs of seg_len-aligned segments)
 *   [5]  big_list    n_keys keys: buckets of 17 .. 2048 runs from the front, of more from the back
 *   [6]  big_count   the two lengths                         [7]  partials  one XYZZ row per run of every bucket of >= 2 runs
 *   [8]  buckets     n_keys XYZZ rows (after the run: the bucket sums)
 *   [9]  n (entries per window the plan was created for)     [10] n_api (points)   [11] c   [12] nwin   [13] B = 2^(c-1)
 *   [14] glv (split-scalar plan)   [15] pre (fixed-base plan)   [16] wide   [17] pw_first   [18] pw_count
 *   [19] w_first, [20] w_count (windows of the last run)     [21] groups (bucket sets)   [22] seg_len   [23] m   [24] dstride
 *        (slots 19-23 describe the last run whatever it was; after zk_msm_plan_enqueue_shared the entry list that run read is the
 *        LENDER's: slots 2-6, 24-27 still describe this plan's own last sort)
 *   [25] sort route (ZK_MSM_ROUTE_*; of the plan's own last sort: a run on a borrowed sort leaves it unchanged)
 *   [26] fine_log (fine bucket bits of the two-level routes, else 0)   [27] split_fine (fine bits kept beside the entries)
 *   [28] 1 when the accumulate kernel of the next run would be the lane-pair one (option split_pairs) */
#define ZK_MSM_VIEW_SLOTS 29
#define ZK_MSM_ROUTE_NONE 0               /* the plan has not sorted yet */
#define ZK_MSM_ROUTE_RANGED 1             /* bucket-range partition */
#define ZK_MSM_ROUTE_ONE_LEVEL 2          /* chunked histogram / prefix / scatter */
#define ZK_MSM_ROUTE_TWO_LEVEL_DERIVE 3   /* two-level, level-A offsets derived in the scatter kernel */
#define ZK_MSM_ROUTE_TWO_LEVEL_SCAN 4     /* two-level, one-workgroup scan of the count matrix */
#define ZK_MSM_ROUTE_TWO_LEVEL_PARTIAL 5  /* two-level, sliced partial sums + scan of the totals + prefix */
int zk_msm_plan_debug_view(uint64_t handle, uint64_t* out, int cap);

/* ---- single-point host arithmetic (PointG1 / PointG2 methods, src/bn254/curve.rs:25-324) -- */

int zk_point_add(int curve, int group, const uint64_t* a, const uint64_t* b, uint64_t* out);      /* __add__ */
int zk_point_neg(int curve, int group, const uint64_t* a, uint64_t* out);                          /* __neg__ */
/* sum of n affine points with one final inversion (the cross-rank combination of MSM partials) */
int zk_point_sum(int curve, int group, uint64_t n, const uint64_t* points, uint64_t* out);
int zk_point_mul(int curve, int group, const uint64_t* a, const uint64_t* scalar, uint64_t* out);  /* __mul__ */
int zk_point_on_curve(int curve, int group, const uint64_t* a);                                    /* 1 / 0 */
int zk_point_generator(int curve, int group, uint64_t* out);                                       /* g1() / g2() */
/* to_bytes / from_bytes = ark-serialize compressed (curve.rs:127-146): 32/64 B (BN254), 48/96 B (BLS12-381).
 * Compression takes reduced coordinates: a coordinate of p or above is refused with ZK_ERR_POINT ("point coordinates are
 * not reduced field elements"), in zk_points_compress too.  A refused call, of either direction and of either form,
 * leaves the caller's out buffer as it was. */
int zk_point_compress(int curve, int group, const uint64_t* a, uint8_t* out);
int zk_point_decompress(int curve, int group, const uint8_t* in, uint64_t* out);

/* The same for the point vectors of a key file (python/zksnake/groth16/serialization.py:60-141 loops to_bytes /
 * from_hex over tau_1, tau_2, target_1, kdelta_1; plonk/serialization.py likewise): n points, one per GPU lane,
 * between host buffers of n * zk_point_limbs words and n * zk_point_bytes bytes.  Decoding validates like
 * zk_point_decompress (flags, x < p, on the curve, prime-order subgroup).  On ZK_ERR_POINT the message is that of the
 * FIRST offending point and *bad_index (may be NULL) its index. */
int zk_points_compress(int curve, int group, uint64_t n, const uint64_t* points, uint8_t* out, uint64_t* bad_index);
int zk_points_decompress(int curve, int group, uint64_t n, const uint8_t* in, uint64_t* out, uint64_t* bad_index);
int zk_point_bytes(int curve, int group);

/* ---- PlonK prover, device-resident vector kernels (csrc/plonk.hip; the generic zk_vec_* among them, which the other
 * provers call too, in csrc/frvec.hip) ----
 * They replace the element-wise polynomial arithmetic of Plonk.prove (python/zksnake/plonk/protocol.py:213-460: chains of
 * fft / mul_over_evaluation_domain / add_over_evaluation_domain, Polynomial scalar multiply-adds, Polynomial.__call__).
 * Vectors are canonical Fr elements in device memory; scalars are canonical 4-limb integers in host memory. */
/* out = a*x + b*y + c (element-wise; b and d_y may both be NULL, c may be NULL); out may alias x or y */
int zk_vec_axpby_dev(int curve, uint64_t n, const uint64_t* a, const void* d_x, const uint64_t* b, const void* d_y, const uint64_t* c,
                     void* d_out, void* stream);
/* acc[i] += sum_{t<k} scalars[t] * x_t[i] for i < counts[t] (counts[t] <= n_acc), then acc[at_index[j]] += at_vals[j] for j < n_at: a chain
 * of Polynomial scalar-multiply-adds and single-coefficient updates (plonk/protocol.py:319-402, :213-236 blinding) in ONE launch -- as
 * separate launches of a few microseconds each they leave the GPU idle between them.  k <= 16, n_at <= 8; scalars / at_vals are 4-limb
 * canonical integers in host memory, k * 4 and n_at * 4 limbs. */
int zk_vec_lincomb_dev(int curve, uint64_t n_acc, void* d_acc, int k, const uint64_t* counts, const void* const* d_x, const uint64_t* scalars,
                       int n_at, const uint64_t* at_index, const uint64_t* at_vals, void* stream);
/* dst[i] = src[offset + i*stride], i < n: one column of the flat witness [a0, b0, c0, a1, ...] (protocol.py:167-169) */
int zk_vec_gather_dev(int curve, uint64_t n, const void* d_src, uint64_t stride, uint64_t offset, void* d_dst, void* stream);
/* *is_zero = 1 when all n elements are zero (synchronises the stream) */
int zk_vec_is_zero_dev(int curve, uint64_t n, const void* d_x, int* is_zero, void* stream);
/* out = sum_i coeffs[i] x^i (Polynomial.__call__, src/bn254/polynomial.rs:491-516); synchronises the stream */
int zk_poly_eval_dev(int curve, uint64_t n, const void* d_coeffs, const uint64_t* x, uint64_t* out, void* stream);
/* k evaluations, polynomial i at xs[i] (4 limbs each) into outs[i], with a single synchronisation (the five opening values
 * and PI(zeta) of a PlonK proof, protocol.py:400-420) */
int zk_poly_eval_many_dev(int curve, int k, const uint64_t* counts, const void* const* d_coeffs, const uint64_t* xs, uint64_t* outs,
                          void* stream);
/* out[i] = prod_{j<3} (wires[j][i] + beta*labels[j][i] + gamma): numerator / denominator terms of the grand product
 * (protocol.py:270-292), labels = the identity or the sigma columns on the n-domain */
int zk_plonk_perm_terms_dev(int curve, uint64_t n, const void* const* d_wires, const void* const* d_labels, const uint64_t* beta,
                            const uint64_t* gamma, void* d_out, void* stream);
/* d_out (n + 1 elements): out[0] = 1, out[i+1] = out[i] * num[i] / den[i] -- the batch_modinv + accumulator loop of
 * protocol.py:296-307 as two product scans, one inversion and one element-wise pass.  ZK_ERR_ARG on a zero denominator. */
int zk_plonk_grand_product_dev(int curve, uint64_t n, const void* d_num, const void* d_den, void* d_out, void* stream);
/* coeffs (n) = q (n - 1 elements, device) * (X - root) + rem (host): Polynomial.__truediv__ by a linear factor
 * (src/bn254/polynomial.rs:404-438) as a geometric rescale, a suffix-sum scan and a rescale back; d_q may not alias d_coeffs */
int zk_poly_div_linear_dev(int curve, uint64_t n, const void* d_coeffs, const uint64_t* root, void* d_q, uint64_t* rem, void* stream);
/* Quotient evaluations on a coset of size m = k*n (2 <= k <= 16) (protocol.py:309-347 evaluated pointwise):
 * out = [gate + alpha*(prod(w_j + beta*k_j*x + gamma)*z - prod(w_j + beta*sigma_j + gamma)*z(omega x)) + alpha^2*(z - 1)*L1] / (x^n - 1)
 * d_cols = 15 vectors of m elements: a, b, c, z, PI, qL, qR, qO, qM, qC, sigma1, sigma2, sigma3, x (the coset points), L1;
 * z(omega x) is read from z at index (i + k) mod m; zh_inv = the k distinct values of 1/(x^n - 1) (host, canonical). */
int zk_plonk_quotient_dev(int curve, uint64_t m, uint64_t n, const void* const* d_cols, const uint64_t* zh_inv, const uint64_t* beta,
                          const uint64_t* gamma, const uint64_t* alpha, void* d_out, void* stream);

/* ---- multilinear polynomials and the sumcheck prover's round (csrc/mle.hip) --------------------------------------
 * A polynomial in log_n variables is the table of its 2^log_n evaluations over {0,1}^log_n: canonical Fr elements in device
 * memory.  Variable 0 is the LEAST significant bit of the table index (ark-poly's order, which GkrPolynomial.to_evaluations
 * relies on: idx = (c << nb) | b), so fixing variable 0 to r is out[j] = in[2j] + r*(in[2j+1] - in[2j]).  Scalars are canonical
 * 4-limb integers in host memory, reduced on entry when >= r.  0 <= log_n <= 40.  ZK_ERR_ARG on bad sizes or overlapping
 * buffers (nothing is written then), ZK_ERR_HIP without a GPU.
 * ZK_MLE_TILE_LOG: a workgroup holds a tile of 2^ZK_MLE_TILE_LOG contiguous elements in LDS and folds up to that many variables
 * per launch, so a k-variable fix reads the table ceil(k / ZK_MLE_TILE_LOG) times (each pass on a table 2^ZK_MLE_TILE_LOG times
 * smaller), not k times. */
#define ZK_MLE_TILE_LOG 8
/* Fix variables 0 .. k-1 to r[0 .. k-1] (k * 4 limbs): MultilinearPolynomial.partial_evaluate (src/bn254/mle.rs:86-91,
 * SparseMultilinearExtension::fix_variables).  d_out receives 2^(log_n - k) elements and must not overlap d_in, which is left
 * unchanged; k = 0 is a copy, k > log_n is ZK_ERR_ARG.  Enqueues only when k <= ZK_MLE_TILE_LOG; a longer chain keeps its
 * intermediate tables in library memory and synchronises the stream before it returns. */
int zk_mle_fix_dev(int curve, int log_n, const void* d_in, int k, const uint64_t* r, void* d_out, void* stream);
/* out (4 limbs, host) = the sum of the n elements of d_x: sum(mlpoly.to_evaluations()) of sumcheck.py:70,108.  Two levels of
 * fixed-order partial sums (exact and repeatable); synchronises the stream. */
int zk_mle_sum_dev(int curve, uint64_t n, const void* d_x, uint64_t* out, void* stream);
/* out (4 limbs, host) = the polynomial at point[0 .. log_n-1] (point[i] goes to variable i): MultilinearPolynomial.evaluate
 * (mle.rs:48-57) as a fix of every variable and a one-element download.  d_x is left unchanged.  d_work: device scratch of at
 * least 2^(max(log_n - ZK_MLE_TILE_LOG, 0) + 1) elements that does not overlap d_x, or NULL to use library memory.
 * Synchronises the stream. */
int zk_mle_eval_dev(int curve, int log_n, const void* d_x, const uint64_t* point, uint64_t* out, void* d_work, void* stream);
/* Evaluations -> monomial coefficients, MultilinearPolynomial.to_coefficients (the recursion ext of mle.rs:9-23): for every
 * bit b, x[i | 1 << b] -= x[i]; entry i is the coefficient of prod_{b in i} x_b.  ZK_MLE_TILE_LOG bits in the first launch, 6 in
 * each later one.  d_out == d_in (in place) or no overlap at all. */
int zk_mle_coeffs_dev(int curve, int log_n, const void* d_in, void* d_out, void* stream);
/* out[j] = in[i] where bit t of j is bit perm[t] of i (perm: log_n bytes, host): permute_evaluations (mle.rs:59-84), and
 * swap(a, b, k) (mle.rs:103-107, ark-poly's relabel) with perm = the identity except perm[a+i] = b+i, perm[b+i] = a+i for i < k.
 * ZK_ERR_ARG unless perm is a permutation of 0 .. log_n-1; d_out must not overlap d_in. */
int zk_mle_permute_dev(int curve, int log_n, const void* d_in, const uint8_t* perm, void* d_out, void* stream);
/* One round of the sumcheck prover (sumcheck.py:49-58 _to_univariate inside :77-92 / :115-126; gkr.py:60-80) for
 *   f(x) = sum_{t < n_terms} term_coeff[t] * prod_{j < term_deg[t]} M_{term_tables[3t + j]}(x),
 * 1 <= term_deg[t] <= 3 (the reference interpolates the round polynomial on a 4-point domain, sumcheck.py:51, gkr.py:75),
 * n_terms <= 8, n_tables <= 8, every table over the same log_n variables; a table may appear in several terms or more than once
 * in one term.  term_coeff: n_terms * 4 limbs; term_tables: n_terms rows of 3 table indices (entries past term_deg[t] ignored).
 * r == NULL:  s_out (4 * 4 limbs, host) = s(X) = sum over x' in {0,1}^(log_n-1) of f(X, x') at X = 0, 1, 2, 3.
 * r given (log_n >= 1): variable 0 of every table is first fixed to r, the folded tables (2^(log_n-1) elements each) are written
 *   to d_tables_out[i], and s_out is s(.) of the FOLDED tables, accumulated in the same pass: a sumcheck round reads each table
 *   once instead of twice.  The folded tables equal what the fix entry point gives for k = 1.  No d_tables_out[i] may overlap
 *   an input table or another output.
 * Tables with no variable left (log_n = 0, or log_n = 1 with r) are constants: s_out is f, four times.
 * Per-workgroup partial sums are added in a fixed order by a second one-workgroup kernel (exact and repeatable).
 * Synchronises the stream. */
int zk_sumcheck_round_dev(int curve, int log_n, int n_tables, const void* const* d_tables, int n_terms, const uint64_t* term_coeff,
                          const int* term_deg, const int* term_tables, const uint64_t* r, void* const* d_tables_out, uint64_t* s_out,
                          void* stream);

/* ---- inner-product argument, scalar side (csrc/ipa.hip) ---------------------------------------------------------------
 * The Bulletproofs halving argument of subprotocol/bulletproofs/ipa.py WITHOUT folding the generators.  n = 2^log_n,
 * 0 <= log_n <= ZK_IPA_MAX_LOG.  After k rounds with challenges u_0 .. u_(k-1) the reference's folded generators are
 *   G^(k)_j = sum_{i = j mod m} s_i G_i,  H^(k)_j = sum_{i = j mod m} s_i^-1 H_i,  m = n >> k,
 *   s_i = prod_{t<k} (bit (log_n-1-t) of i ? u_t : u_t^-1)       (the verifier's s vector once k = log_n),
 * so L_k and R_k are MSMs over the ORIGINAL G || H (2n bases, one plan for a whole proof) with the scalars written here.
 * All vectors are canonical Fr elements in device memory; challenges are canonical 4-limb integers in host memory, reduced
 * on entry when >= r.  Workgroups of 256 threads on a grid capped at 1024 workgroups: the pass over i < n takes a second item
 * per thread first at n = 2^19, the fold (m items) and the cross products (m/2 items) first at n = 2^20.
 * ZK_ERR_ARG for a null pointer, sizes out of range, a challenge missing or present against the rules below, or two buffers
 * that overlap; nothing is written then. */
#define ZK_IPA_MAX_LOG 22
/* Round k of the prover, 0 <= k <= log_n; m = n >> k, h = m / 2.  d_a, d_b: n elements, of which the first 2m are live on
 * entry (n when k = 0) and the first m afterwards; d_s, d_s_inv: n elements; d_scal_L, d_scal_R: 2n elements each.
 * Step 1.  k = 0: u and u_inv must be NULL; s[i] = s_inv[i] = 1.  k >= 1: u, u_inv (4 limbs each) are the challenge of round
 *   k-1 and its inverse (u * u_inv = 1 is not checked); in place for j < m
 *     a[j] = u a[j] + u_inv a[j+m],   b[j] = u_inv b[j] + u b[j+m],
 *   then for i < n with bit = (i >> (log_n - k)) & 1:  s[i] *= bit ? u : u_inv,  s_inv[i] *= bit ? u_inv : u.
 * Step 2 (k < log_n only), for i < n with j = i mod m:
 *     j >= h:  scal_L[i] = a[j-h] s[i],  scal_R[n+i] = b[j-h] s_inv[i],  scal_L[n+i] = scal_R[i] = 0
 *     j <  h:  scal_L[n+i] = b[j+h] s_inv[i],  scal_R[i] = a[j+h] s[i],  scal_L[i] = scal_R[n+i] = 0
 *   (every element of d_scal_L, d_scal_R is written, zeros included), so that
 *     L_k = <scal_L, G || H> + cross[0..3] Q,   R_k = <scal_R, G || H> + cross[4..7] Q,
 *     cross[0..3] = sum_{j<h} a[j] b[j+h],   cross[4..7] = sum_{j<h} a[j+h] b[j]   (host, canonical; fixed-order sums).
 * With k == log_n only step 1 runs: d_scal_L, d_scal_R and cross may be NULL and are not touched; a[0], b[0] are the proof's
 * scalars.  Synchronises the stream when it returns cross (k < log_n), otherwise it only enqueues. */
int zk_ipa_round_dev(int curve, int log_n, int k, void* d_a, void* d_b, void* d_s, void* d_s_inv, const uint64_t* u,
                     const uint64_t* u_inv, void* d_scal_L, void* d_scal_R, uint64_t* cross, void* stream);
/* The verifier's scalars (ipa.py:189-198) for the proof's a, b (4 limbs each, host) and the challenges u, u_inv (log_n * 4 limbs
 * each, host; may be NULL when log_n = 0): d_out[i] = a s_i, d_out[n+i] = b s_i^-1 for i < n, 2n elements, log_n products per
 * element.  log_n = 0 gives [a, b].  Enqueues only. */
int zk_ipa_verify_scalars_dev(int curve, int log_n, const uint64_t* u, const uint64_t* u_inv, const uint64_t* a, const uint64_t* b,
                              void* d_out, void* stream);
/* zk_ipa_round_dev with a weighted H side: at k = 0 with d_h_weight non-NULL (n canonical elements, read only, part of the
 * overlap check) s_inv[i] = h_weight[i] instead of 1, so that every later round and the verifier's H scalars carry the weight:
 * the argument then runs over H'_i = h_weight[i] H_i without H' ever being formed (a range proof passes y^-i).  For k >= 1
 * d_h_weight must be NULL (ZK_ERR_ARG otherwise); with NULL this is zk_ipa_round_dev. */
int zk_ipa_round_seeded_dev(int curve, int log_n, int k, void* d_a, void* d_b, void* d_s, void* d_s_inv, const void* d_h_weight,
                            const uint64_t* u, const uint64_t* u_inv, void* d_scal_L, void* d_scal_R, uint64_t* cross, void* stream);

/* ---- Bulletproofs range proof, scalar side (csrc/rangeproof.hip) --------------------------------------------------------
 * subprotocol/bulletproofs/range_proof.py for m values of n bits in one argument over N = n m positions (the reference has
 * m = 1): n = 2^log_bits, N = 2^log_N, 0 <= log_bits <= 7, log_bits <= log_N <= ZK_IPA_MAX_LOG.  Position k = j n + i is bit i of
 * value j.  d_values: m x 2 64-bit limbs in device memory, the low 128 bits of each value, low limb first; bits at or above n
 * are ignored.  Vectors are canonical Fr elements in device memory; y, y_inv, z, x, a, b, u, u_inv are canonical 4-limb
 * integers in host memory, reduced on entry when >= r.  With
 *     a_L[k] = bit i of v_j,  a_R = a_L - 1,  l0 = a_L - z,  l1 = s_L,
 *     r0[k] = y^k (a_R[k] + z) + z^(2+j) 2^i,  r1[k] = y^k s_R[k]
 * the prover's entry points write the scalars of A, the coefficients of t(X) = <l0 + l1 X, r0 + r1 X>, and l, r at X = x.
 * y^k, y_inv^k and z^(2+j) are built per thread from the squarings g^(2^t), t <= 18, which travel as kernel arguments, and step
 * by g^(2^18) per grid-stride item; 2^i is the integer with bit i set.  Workgroups of 256 threads on a grid capped at 1024
 * workgroups: a thread takes a second item first at N = 2^19.  ZK_ERR_ARG for a null pointer, sizes out of range, an unknown
 * curve or an output that overlaps another buffer of the call; nothing is written then. */
/* d_out (2N elements) = a_L || a_R: out[k] in {0, 1}, out[N+k] = a_L[k] ? 0 : r-1.  Enqueues only. */
int zk_rp_bits_dev(int curve, int log_bits, int log_N, const void* d_values, void* d_out, void* stream);
/* t_out (12 limbs, host) = t0 = <l0, r0>, t1 = <l0, r1> + <l1, r0>, t2 = <l1, r1>.  d_s = s_L || s_R, 2N elements, read only.
 * One pass, three fixed-order sums (exact and repeatable); l0, r0 are not stored.  Synchronises the stream. */
int zk_rp_poly_dev(int curve, int log_bits, int log_N, const void* d_values, const void* d_s, const uint64_t* y, const uint64_t* z,
                   uint64_t* t_out, void* stream);
/* d_ab[k] = l[k] = l0[k] + x l1[k], d_ab[N+k] = r[k] = r0[k] + x r1[k] (2N elements: the a || b of the inner-product argument),
 * d_h_weight[k] = y_inv^k (N elements: the weights of zk_ipa_round_seeded_dev).  y * y_inv = 1 is not checked.  Enqueues only. */
int zk_rp_eval_dev(int curve, int log_bits, int log_N, const void* d_values, const void* d_s, const uint64_t* y, const uint64_t* y_inv,
                   const uint64_t* z, const uint64_t* x, void* d_ab, void* d_h_weight, void* stream);
/* The verifier's scalars of G || H (range_proof.py:273-280) with s_k the s vector of the inner-product argument above:
 * d_out[k] = -z - a s_k,  d_out[N+k] = z + y_inv^k (z^(2+j) 2^i - b s_k^-1), 2N elements.  u, u_inv: log_N * 4 limbs each (may
 * be NULL when log_N = 0).  Enqueues only. */
int zk_rp_verify_scalars_dev(int curve, int log_bits, int log_N, const uint64_t* u, const uint64_t* u_inv, const uint64_t* a,
                             const uint64_t* b, const uint64_t* y_inv, const uint64_t* z, void* d_out, void* stream);

/* ---- inner-product polynomial commitment, scalar side of an opening (csrc/pcs.hip) ----------------------------------------
 * The halving argument of commitment/polynomial/ipa.py (BCMS20 appendix A) WITHOUT folding the generators and without a b
 * vector.  It is not the argument of csrc/ipa.hip: one generator vector G, asymmetric folds c' = c_lo + u^-1 c_hi,
 * G' = G_lo + u G_hi, b' = b_lo + u b_hi, and b = (1, z, z^2, ..) for the opening point z.  n = 2^log_n,
 * 0 <= log_n <= ZK_PCS_MAX_LOG.  After k rounds with challenges u_0 .. u_(k-1), m = n >> k:
 *   G^(k)_j = sum_{i = j mod m} s_i G_i,   s_i = prod_{t<k} (bit (log_n-1-t) of i ? u_t : 1),
 *   b^(k)_j = B_k z^j,                     B_k = prod_{t<k} (1 + u_t z^(n >> (t+1)))   (one scalar, kept by the caller),
 * so L_k and R_k are MSMs over the ORIGINAL G (n bases, one plan for a whole opening) with the scalars written here, plus the
 * caller's B_k times an evaluation at z of half of c.  Vectors are canonical Fr elements in device memory; u, u_inv, z, c are
 * canonical 4-limb integers in host memory, reduced on entry when >= r.  z^j is built per thread from the squarings z^(2^t),
 * t <= 18, which travel as kernel arguments, and steps by z^(2^18) per grid-stride item.  Workgroups of 256 threads on a grid
 * capped at 1024 workgroups: the pass over i < n takes a second item per thread first at n = 2^19, the fold (m items) and the
 * evaluations (m/2 items) first at n = 2^20.  ZK_ERR_ARG for a null pointer, sizes out of range, an unknown curve, a challenge
 * missing or present against the rules below, or two buffers that overlap; nothing is written then. */
#define ZK_PCS_MAX_LOG 21
/* Round k of an opening, 0 <= k <= log_n; m = n >> k, h = m / 2.  d_c: n elements, of which the first 2m are live on entry (n
 * when k = 0) and the first m afterwards; d_s, d_scal_L, d_scal_R: n elements each.
 * Step 1.  k = 0: u and u_inv must be NULL; s[i] = 1.  k >= 1: u, u_inv (4 limbs each) are the challenge of round k-1 and its
 *   inverse (u * u_inv = 1 is not checked); in place for j < m
 *     c[j] += u_inv c[j+m],
 *   then for i < n with bit (log_n - k) of i set:  s[i] *= u.
 * Step 2 (k < log_n only; z, 4 limbs, is the opening point), for i < n with j = i mod m:
 *     j <  h:  scal_L[i] = c[j+h] s[i],  scal_R[i] = 0
 *     j >= h:  scal_R[i] = c[j-h] s[i],  scal_L[i] = 0
 *   (every element of d_scal_L, d_scal_R is written, zeros included), so that with h' the argument's second generator
 *     L_k = <scal_L, G> + B_k evals[0..3] h',   R_k = <scal_R, G> + B_k z^h evals[4..7] h',
 *     evals[0..3] = sum_{j<h} c[j+h] z^j,   evals[4..7] = sum_{j<h} c[j] z^j   (host, canonical; exact fixed-order sums).
 * With k == log_n only step 1 runs: z, d_scal_L, d_scal_R and evals may be NULL and are not touched; c[0] is the proof's scalar.
 * Synchronises the stream when it returns evals (k < log_n), otherwise it only enqueues. */
int zk_pcs_round_dev(int curve, int log_n, int k, void* d_c, void* d_s, const uint64_t* u, const uint64_t* u_inv, const uint64_t* z,
                     void* d_scal_L, void* d_scal_R, uint64_t* evals, void* stream);
/* The verifier's scalars for the proof's c (4 limbs, host) and the challenges u (log_n * 4 limbs, host; may be NULL when
 * log_n = 0): d_out[i] = c s_i for i < n with s_i as above for k = log_n -- the coefficients of the reference's
 * g(X) = prod_i (1 + u_(log_n-1-i) X^(2^i)), times c -- n elements, at most log_n products per element.  log_n = 0 gives [c].
 * Enqueues only. */
int zk_pcs_verify_scalars_dev(int curve, int log_n, const uint64_t* u, const uint64_t* c, void* d_out, void* stream);

/* ---- multilinear KZG commitment, scalar side of an opening (csrc/mlpcs.hip) ------------------------------------------------
 * PST13 multilinear KZG as in arkworks' MultilinearPC, over the tables of csrc/mle.hip (variable 0 is the least significant bit of
 * the index, point[i] goes to variable i).  Opening f at z is the chain, from f_0 = f and for k = 0 .. log_n-1,
 *     q_k[b] = f_k[2b+1] - f_k[2b],     f_(k+1)[b] = f_k[2b] + z_k q_k[b],
 * so that f(x) - f(z) = sum_k (x_k - z_k) q_k(x_(k+1), ..) and f_(log_n)[0] = f(z): the q_k are the scalars of the proof's log_n
 * MSMs and the evaluation comes out of the same pass.  0 <= log_n <= ZK_MLPCS_MAX_LOG (the commitment scheme's cap: its SRS holds
 * 2^(log_n + 1) points).  Tiled like zk_mle_fix_dev: ceil(log_n / ZK_MLE_TILE_LOG) launches, each on a table 2^ZK_MLE_TILE_LOG
 * times smaller; every quotient is written once. */
#define ZK_MLPCS_MAX_LOG 24
/* d_f: 2^log_n canonical Fr elements, left unchanged.  point: log_n * 4 limbs (host; may be NULL when log_n = 0), reduced on
 * entry when >= r.  d_q receives all 2^log_n - 1 quotient entries (canonical), level 0 first: level k has 2^(log_n-1-k) entries and
 * starts at element 2^log_n - 2^(log_n-k).  eval_out (4 limbs, host) = f(point).  d_work: device scratch of at least
 * 2^(max(log_n - ZK_MLE_TILE_LOG, 0) + 1) elements, or NULL to use library memory (the zk_mle_eval_dev convention).  log_n = 0
 * writes no quotient (d_q may be NULL) and returns f[0].  ZK_ERR_ARG, with nothing written, for a null pointer, log_n out of
 * range, an unknown curve, d_q overlapping d_f, or d_work overlapping either; ZK_ERR_HIP without a GPU.  Synchronises the stream. */
int zk_mlpcs_quotients_dev(int curve, int log_n, const void* d_f, const uint64_t* point, void* d_q, uint64_t* eval_out, void* d_work,
                           void* stream);

/* ---- Merkle vector commitment: BLAKE2b leaves, tree and opening paths (csrc/merkle.hip) ----------------------------------
 * The hashing of commitment/vector/merkle.py with alg = "blake2b": BLAKE2b-512 without key, salt or personalisation (RFC 7693,
 * what hashlib.new("blake2b", data) computes), one digest per lane.  A tree over n leaves is its levels one after the other in
 * device memory, ZK_MERKLE_DIGEST bytes per node: level 0 (the n leaf digests) first, level l has ceil(n_(l-1) / 2) nodes, the
 * root is the last node; depth = ceil(log2 n), and n = 1 is depth 0 with the root equal to the leaf digest.  Parent i of a level
 * is H(child[2i] || child[2i+1]), with child[2i] in the place of a right sibling that does not exist (the reference's
 * _build_tree).  Workgroups of 256 threads on a grid capped at 1024 workgroups: a pass takes a second item per thread first
 * past 2^18 items.  Digests, trees and paths start at a multiple of 16 bytes, offsets and indices at a multiple of 8.
 * ZK_ERR_ARG, before anything is launched, for n = 0 or n > 2^ZK_MERKLE_MAX_LOG, a null pointer (d_rows / d_data may be NULL
 * when there are no bytes to read), a misaligned one, row_bytes >= 2^32 or an output that overlaps an input.  No entry point
 * allocates device memory; all of them only enqueue on `stream`. */
#define ZK_MERKLE_DIGEST 64
#define ZK_MERKLE_MAX_LOG 26     /* at most 2^26 leaves, the MSM plans' point limit: 4 GiB of leaf digests, < 8 GiB of tree */
/* d_digests[i] = BLAKE2b(the row_bytes bytes at d_rows + i * row_bytes), i < n.  64-bit loads when d_rows and row_bytes are
 * multiples of 8, byte loads otherwise; row_bytes = 0 gives n digests of the empty message. */
int zk_blake2b_rows_dev(uint64_t n, const void* d_rows, uint64_t row_bytes, void* d_digests, void* stream);
/* The same over items of any lengths: item i is bytes [off[i], off[i+1]) of d_data (data_bytes bytes), d_offsets: n + 1 uint64
 * in device memory.  The kernel clamps end = min(off[i+1], data_bytes), start = min(off[i], end): offsets that are out of range
 * or out of order give the digests of the clamped ranges and never a read outside d_data. */
int zk_blake2b_items_dev(uint64_t n, const void* d_data, uint64_t data_bytes, const void* d_offsets, void* d_digests, void* stream);
/* Host arithmetic only (works without a GPU): depth, the first node of every level (depth + 1 entries, room for
 * ZK_MERKLE_MAX_LOG + 1) and the number of nodes.  Each output may be NULL. */
int zk_merkle_layout(uint64_t n, int* depth, uint64_t* level_offset /* ZK_MERKLE_MAX_LOG + 1 entries, in nodes */, uint64_t* nodes);
/* Levels 1 .. depth of d_tree (`nodes` nodes) from level 0, which the caller has put at its front; level 0 is not written. */
int zk_merkle_build_dev(uint64_t n, void* d_tree, void* stream);      /* level 0 already in place at the front of d_tree */
/* d_paths: k * depth nodes; entry (q, l) is the sibling of the level-l ancestor of leaf d_indices[q]: node idx ^ 1 of that level,
 * or node idx itself where idx ^ 1 is past the level (the copy its parent was hashed from), so that the reference's verify loop
 * accepts every path.  An index >= n opens leaf n - 1.  One gather; k = 0 is ZK_OK and launches nothing, as is depth = 0. */
int zk_merkle_paths_dev(uint64_t n, const void* d_tree, uint64_t k, const void* d_indices /* k uint64 */, void* d_paths, void* stream);

/* ---- Poseidon over Fr: permutation, fixed-length hash, sponge over rows and Merkle trees (csrc/poseidon.hip) -----------------
 * Poseidon (Grassi et al., USENIX Security 2021) with S-box x^5 over Fr of either curve, state width t in {3, 4, 5}, R_F = 8 and
 * R_P = 57 / 56 / 60 (circomlib's table, on both curves).  A round: add the round constants, S-box (every element in the first and
 * last R_F / 2 rounds, element 0 in between), then state_i = sum_j M[i][j] state_j.  Round constants and M = 1 / (x_i + y_j) come
 * from the paper's Grain LFSR; the library generates them on the host at first use and keeps one device
 * table per (curve, t) until zk_shutdown.
 *   perm_t             the permutation
 *   hash(x_1..x_k)     perm_(k+1)([0, x_1, .., x_k])[0], k in {2, 3, 4}: circomlib's Poseidon(k)
 *   sponge(row), L >= 1 elements: t = 3, the state starts as [L, 0, 0]; block i adds row[2i] to state[1] and row[2i+1], where it
 *                      exists, to state[2]; perm_3 after every block; the digest is state[1]
 *   tree               level 0 is n digests, parent = hash(left, right), a node without a right sibling is hashed with itself:
 *                      the shape zk_merkle_layout describes, ZK_POSEIDON_NODE = 32 bytes per node (one canonical element)
 * All inputs are canonical Fr elements (32 bytes) in device memory.  One permutation per lane, workgroups of 256 threads on a
 * grid capped at 1024 workgroups: a pass takes a second item per thread first past 2^18 items.  ZK_ERR_ARG, before anything is
 * launched or written, for n = 0 or n > 2^ZK_POSEIDON_MAX_LOG, a t, k or curve that does not exist, a null pointer, a vector that
 * does not start at a multiple of 16 (indices: of 8) or an output that overlaps an input.  No entry point allocates beyond the
 * parameter table; all of them only enqueue on `stream`. */
#define ZK_POSEIDON_MAX_LOG 26
#define ZK_POSEIDON_MAX_ROW (1u << 20)
/* Host only (works without a GPU): *rf = R_F, *rp = R_P, out = the (R_F + R_P) t round constants in round order (constant
 * [round][i] is added to state[i]) and then the t * t entries of M row-major, canonical 4-limb values.  Each output may be NULL. */
int zk_poseidon_params(int curve, int t, int* rf, int* rp, uint64_t* out);
/* state i (t elements at d_in + i t) -> perm_t of it at d_out + i t, i < n.  d_out == d_in is allowed, any other overlap is not. */
int zk_poseidon_perm_dev(int curve, int t, uint64_t n, const void* d_in, void* d_out, void* stream);
/* d_out[i] = hash(the k elements at d_rows + i k), i < n */
int zk_poseidon_hash_dev(int curve, int k, uint64_t n, const void* d_rows, void* d_out, void* stream);
/* d_digests[i] = sponge(the row_elems elements at d_rows + i row_elems), i < n; 1 <= row_elems <= ZK_POSEIDON_MAX_ROW */
int zk_poseidon_sponge_rows_dev(int curve, uint64_t n, const void* d_rows, uint64_t row_elems, void* d_digests, void* stream);
/* Levels 1 .. depth of d_tree (`nodes` nodes of 32 bytes) from level 0, which the caller has put at its front; n = 1 launches nothing. */
int zk_poseidon_merkle_build_dev(int curve, uint64_t n, void* d_tree, void* stream);
/* zk_merkle_paths_dev on 32-byte nodes, the same gather and the same rules: d_paths is k * depth nodes. */
int zk_poseidon_merkle_paths_dev(uint64_t n, const void* d_tree, uint64_t k, const void* d_indices /* k uint64 */, void* d_paths, void* stream);

/* ---- FRI polynomial commitment: low-degree extension, fold and row gather (csrc/fri.hip) ------------------------------------
 * The device side of commitment/polynomial/fri.py (the reference has no FRI).  A layer f of M = 2h canonical Fr elements on a
 * coset s <w> (w of order M) is stored in PAIR ORDER: g[2j] = f[j], g[2j+1] = f[j+h] for j < h, the values at x_j = s w^j and at
 * -x_j, so that leaf j of the layer's Merkle tree is the 64 bytes at g + 64 j (zk_blake2b_rows_dev(h, g, 64, ..)).  A layer of
 * one element is that element.  Vectors are canonical Fr elements in device memory and start at a multiple of 16 bytes;
 * scalars are canonical 4-limb integers in host memory, reduced on entry when >= r.  Powers are built per thread from the
 * squarings of the scalar, t <= 18, which travel as kernel arguments, and step by its 2^18-th squaring per grid-stride item.
 * Workgroups of 256 threads on a grid capped at 1024 workgroups.  ZK_ERR_ARG, before anything is launched or written, for a
 * null or misaligned pointer, a size out of range, an unknown curve or two buffers of a call that overlap.  All three entry
 * points only enqueue on `stream`, and none allocates device memory (zk_ntt_dev, which zk_fri_lde_dev calls, keeps its twiddle
 * tables in the transform's own cache). */
#define ZK_FRI_MAX_LOG 26            /* a layer has at most 2^26 elements: the domain of the largest polynomial times its blowup */
#define ZK_FRI_MAX_ROW_BYTES 65536   /* zk_fri_rows_dev: bytes per row */
/* d_out (2^(log_n + log_blowup) = N elements) = the polynomial sum_{i < n_coeffs} c_i X^i on the coset shift <w>, w =
 * zk_fr_root_of_unity(N), in pair order: d_work[i] = c_i shift^i for i < n_coeffs and zero for n_coeffs <= i < N, zk_ntt_dev
 * (forward, natural order in and out) in place on d_work, then d_out[2j] = d_work[j], d_out[2j+1] = d_work[j + N/2] for j < N/2.
 * log_n >= 0, log_blowup >= 1, log_n + log_blowup <= ZK_FRI_MAX_LOG, n_coeffs <= 2^log_n; d_coeffs (n_coeffs elements) may be
 * NULL when n_coeffs = 0, which gives N zeros.  d_work: N elements of scratch, holding the natural-order evaluations
 * afterwards.  d_coeffs, d_work and d_out may not overlap one another.  The scale pass takes a second item per thread first at
 * N = 2^19, the permutation (N/2 items, one 64-byte pair each) first at N = 2^20. */
int zk_fri_lde_dev(int curve, int log_n, int log_blowup, uint64_t n_coeffs, const void* d_coeffs, const uint64_t* shift, void* d_work,
                   void* d_out, void* stream);
/* One fold of a layer of M = 2^log_m = 2h elements (d_in, pair order) into the next layer of h elements (d_out, pair order of
 * h values: value j is stored at 2j for j < h/2 and at 2(j - h/2) + 1 otherwise; at h = 1 at 0), 1 <= log_m <= ZK_FRI_MAX_LOG:
 *     value j = (d_in[2j] + d_in[2j+1]) / 2 + c w_inv^j (d_in[2j] - d_in[2j+1]),   j < h,
 * which with c = alpha / (2 s) and w_inv = w^-1 is f'(x_j^2) for f' = f_even + alpha f_odd; the caller inverts 2 s and w once
 * per layer (neither relation is checked).  Each thread reads one 64-byte pair; threads take a second item first at
 * h = 2^19.  d_out may not overlap d_in. */
int zk_fri_fold_dev(int curve, int log_m, const void* d_in, const uint64_t* c, const uint64_t* w_inv, void* d_out, void* stream);
/* d_out (k rows) = rows d_indices[q], q < k, of the n_rows rows of row_bytes bytes at d_rows: the queried leaves of a layer in
 * one launch.  An index >= n_rows takes row n_rows - 1 (as zk_merkle_paths_dev opens the last leaf).  1 <= n_rows <= 2^32;
 * row_bytes is a multiple of 16, 16 <= row_bytes <= ZK_FRI_MAX_ROW_BYTES; k <= 2^32.  d_rows and d_out start at a multiple of
 * 16, d_indices (k uint64, device memory) at a multiple of 8; d_out may not overlap d_rows or d_indices.  k = 0 is ZK_OK and
 * launches nothing (d_indices and d_out may be NULL then; d_rows may not). */
int zk_fri_rows_dev(uint64_t n_rows, uint64_t row_bytes, const void* d_rows, uint64_t k, const void* d_indices /* k uint64 */, void* d_out,
                    void* stream);

/* ---- GKR over layered circuits, the sparse side (csrc/gkr.hip) ----------------------------------------------------------
 * Layer j of a circuit has n_j wires and a dense table W_j of 2^k_j canonical Fr elements in device memory (zero beyond n_j),
 * 1 <= k_j <= ZK_GKR_MAX_LOG.  Gate g of layer j is (types[g]: 0 ADD / 1 MUL, in1[g], in2[g]) with in1, in2 < n_(j-1): three
 * device arrays (u8, u32, u32) in gate order.  THE CALLER has checked the indices (LayeredCircuit.compile does): the kernels
 * gather W_(j-1)[in1[g]] without a bounds test.  The wiring predicates add_j, mul_j of gkr.py:113-171 have one non-zero entry
 * per gate, at (a, b, c) = (g, in1[g], in2[g]); every entry point below sums over gates instead of over that hypercube.
 * Scalars are canonical 4-limb integers in host memory, reduced on entry when >= r.  Sums are fixed-order (exact and
 * repeatable); no atomics.  ZK_ERR_ARG for a null pointer, a size out of range or an output that overlaps another buffer of
 * the call; nothing is written then. */
#define ZK_GKR_MAX_LOG 24
/* Rows of the two CSRs with more entries than this leave the lane-per-row kernel (spmv.py's LONG_ROW). */
#define ZK_GKR_LONG_ROW 64
/* d_out[g] = types[g] ? W[in1[g]] * W[in2[g]] : W[in1[g]] + W[in2[g]] for g < n_gates, 0 for n_gates <= g < 2^log_out: the table
 * of layer j from the table d_w (2^log_prev elements) of layer j-1 (LayeredCircuit.evaluate, layered_circuit.py:77-104, one
 * layer).  n_gates <= 2^log_out.  Enqueues only. */
int zk_gkr_layer_eval_dev(int curve, uint64_t n_gates, const void* d_types, const void* d_in1, const void* d_in2, int log_prev,
                          const void* d_w, int log_out, void* d_out, void* stream);
/* d_out[x] = eq(r, x) = prod_{t<k} (bit t of x ? r[t] : 1 - r[t]) for x < 2^k; r: k * 4 limbs (NULL when k = 0, which gives [1]).
 * Every element is k products from the challenges, which travel as kernel arguments.  Enqueues only. */
int zk_gkr_eq_table_dev(int curve, int k, const uint64_t* r, void* d_out, void* stream);
/* The two bookkeeping passes of the prover over a CSR of the layer's gates with 2^log_rows rows (log_rows = k_(j-1)):
 * row_ptr (2^log_rows + 1, u32), and per entry gate (the gate's index a, u32), other (the gate's input that is not the row,
 * u32) and types (u8); n_entries = the layer's gates <= 2^log_e.  d_e: E[a] = eq(r, a), 2^log_e elements (log_e = k_j).
 *   phase 1, rows = in1, other = in2, d_w = W_(j-1):   P[b] = sum_ADD E[a] + sum_MUL E[a] W[c],   Q[b] = sum_ADD E[a] W[c]
 *   phase 2, rows = in2, other = in1, d_e2 = eq(u, .): Aadd[c] = sum_ADD E[a] E2[b],              Amul[c] = sum_MUL E[a] E2[b]
 * Both outputs (2^log_rows elements each) come from one pass with one product per gate; every row is written, empty rows as
 * zero.  Rows of more than ZK_GKR_LONG_ROW entries: long_rows (n_long, u32), item_ptr (n_long + 1, u32) and items (n_items pairs
 * [e0, e1) of u32) cut them into work items as spmv.py's long_row_items does; d_partials: 2 * n_items elements of scratch.
 * With n_long = 0 these four may be NULL.  Enqueue only. */
int zk_gkr_phase1_dev(int curve, int log_rows, uint64_t n_entries, const void* d_row_ptr, const void* d_gate, const void* d_other,
                      const void* d_types, uint64_t n_long, const void* d_long_rows, const void* d_item_ptr, uint64_t n_items,
                      const void* d_items, void* d_partials, int log_e, const void* d_e, const void* d_w, void* d_p, void* d_q, void* stream);
int zk_gkr_phase2_dev(int curve, int log_rows, uint64_t n_entries, const void* d_row_ptr, const void* d_gate, const void* d_other,
                      const void* d_types, uint64_t n_long, const void* d_long_rows, const void* d_item_ptr, uint64_t n_items,
                      const void* d_items, void* d_partials, int log_e, const void* d_e, const void* d_e2, void* d_add, void* d_mul,
                      void* stream);
/* out[0..3] = add~_j(r, u, v) = sum over ADD gates of E_r[g] E_u[in1[g]] E_v[in2[g]], out[4..7] = the same over MUL gates (host,
 * canonical): what gkr.py:262-263, :331-332 get from two dense selector polynomials.  d_er: eq(r, .), 2^log_a elements;
 * d_eu, d_ev: eq(u, .), eq(v, .), 2^log_prev elements each.  n_gates <= 2^log_a.  Synchronises the stream. */
int zk_gkr_wiring_eval_dev(int curve, uint64_t n_gates, const void* d_types, const void* d_in1, const void* d_in2, int log_a,
                           const void* d_er, int log_prev, const void* d_eu, const void* d_ev, uint64_t* out, void* stream);

/* ---- Spartan over R1CS: witness products and row binding (csrc/spartan.hip) ------------------------------------------------
 * Both entry points walk a MERGED THREE-MATRIX CSR with n_seg = 2^log_seg segments, 0 <= log_seg <= ZK_R1CS_MAX_LOG:
 * ptr u32[3 n_seg + 1]; sub-segment q = 3 i + m holds the entries of matrix m (0 A, 1 B, 2 C) in segment i, at
 * idx[ptr[q] .. ptr[q+1]) (u32) and val (canonical Fr); n_entries = ptr[3 n_seg] < 2^32.  Padding segments are empty; a repeated
 * (segment, idx) adds.  x is a table of 2^log_x canonical Fr elements and THE CALLER has checked idx < 2^log_x (Spartan's
 * constructor does): the kernels gather x[idx[k]] without a bounds test.  Per segment acc_m = sum_k val[k] x[idx[k]] over
 * sub-segment 3 i + m: one product per entry.
 * Long segments -- those with a sub-segment of more than ZK_R1CS_LONG_ROW entries: long_segs u32[n_long] (ascending segment
 * indices), item_ptr u32[3 n_long + 1] into items (the items of sub-segment m of long segment j are item_ptr[3 j + m] ..
 * item_ptr[3 j + m + 1]: none for a short sub-segment), items u32[n_items][2] = entry ranges [k0, k1) as spmv.py's long_row_items
 * cuts them from ptr, d_partials = n_items elements of scratch.  With n_long = 0 (and then n_items = 0) these four may be NULL.
 * Sums are fixed-order (exact and repeatable); no atomics; every output element is written once, empty sub-segments as zero.
 * ZK_ERR_ARG for a null pointer, log_seg or log_x out of range, n_entries >= 2^32, n_long > n_items, n_items > n_entries,
 * n_long > 2^log_seg, n_items without n_long, a missing long-segment array, or an output (d_partials included) that overlaps
 * another buffer of the call; nothing is written then.  Both enqueue only. */
#define ZK_R1CS_MAX_LOG 24
#define ZK_R1CS_LONG_ROW 64
/* The row-major CSR (segments = constraints, idx = column, x = z): d_az[i], d_bz[i], d_cz[i] = acc_A, acc_B, acc_C for every
 * i < 2^log_seg -- A z, B z and C z from one pass over one index stream. */
int zk_r1cs_products_dev(int curve, int log_seg, uint64_t n_entries, const void* d_ptr, const void* d_idx, const void* d_val,
                         uint64_t n_long, const void* d_long_segs, const void* d_item_ptr, uint64_t n_items, const void* d_items,
                         void* d_partials, int log_x, const void* d_z, void* d_az, void* d_bz, void* d_cz, void* stream);
/* The column-major CSR (segments = columns, idx = constraint, x = E = eq(rx, .)): d_out[y] = cA acc_A + cB acc_B + cC acc_C =
 * sum_i E[i] (cA A + cB B + cC C)[i, y] for every y < 2^log_seg.  coeff: cA, cB, cC, 3 x 4 limbs in host memory, reduced on
 * entry.  One product per entry and three per segment. */
int zk_r1cs_bind_dev(int curve, int log_seg, uint64_t n_entries, const void* d_ptr, const void* d_idx, const void* d_val,
                     uint64_t n_long, const void* d_long_segs, const void* d_item_ptr, uint64_t n_items, const void* d_items,
                     void* d_partials, int log_x, const void* d_e, const uint64_t* coeff, void* d_out, void* stream);

/* Dense-polynomial helpers over Fr used by the PlonK prover (python/zksnake/plonk/protocol.py:157-484); canonical
 * coefficients, lowest degree first, host memory.  They replace Polynomial.__call__ (src/bn254/polynomial.rs:491-516),
 * Polynomial.__truediv__ by a linear factor (:404-438), the batch_modinv + accumulator loop of protocol.py:296-307 and
 * Polynomial scalar-multiply-add chains (:319-402). */
int zk_fr_poly_eval(int curve, uint64_t n, const uint64_t* coeffs, const uint64_t* x, uint64_t* out);
/* coeffs (n) = q (n - 1 entries) * (X - root) + rem (1 entry) */
int zk_fr_poly_div_linear(int curve, uint64_t n, const uint64_t* coeffs, const uint64_t* root, uint64_t* q, uint64_t* rem);
/* out (n + 1 entries): out[0] = 1, out[i+1] = out[i] * num[i] / den[i]; ZK_ERR_ARG on a zero denominator */
int zk_fr_grand_product(int curve, uint64_t n, const uint64_t* num, const uint64_t* den, uint64_t* out);
/* acc[i] += s * x[i], i < n */
int zk_fr_scale_add(int curve, uint64_t n, uint64_t* acc, const uint64_t* x, const uint64_t* s);

/* pairing / multi_pairing (src/bn254/curve.rs:417-437): out = prod_i e(g1[i], g2[i]) after the final exponentiation,
 * as 12 base-field elements (coefficients of 1, w, .., w^5 over Fp2; zk_gt_limbs 64-bit limbs).  Host only. */
int zk_gt_limbs(int curve);
int zk_multi_pairing(int curve, uint64_t n, const uint64_t* g1_points, const uint64_t* g2_points, uint64_t* out);

/* ---- scalar-field host helpers (setup/verify side; polynomial.rs:518-533,636-652) -------- */

int zk_fr_root_of_unity(int curve, uint64_t n, uint64_t* out);                 /* get_evaluation_point(n, 1) */
int zk_fr_lagrange_coeffs(int curve, uint64_t n, const uint64_t* tau, uint64_t* out); /* evaluate_lagrange_coefficients */

#ifdef __cplusplus
}
#endif
#endif /* ZKMI_H */
