// mp4x native C API (CDNA4 / gfx950): the kernels (csrc/kernels/*.hip).
//
// Three plain-C headers ARE the ABI of the native libraries; every exported mp4x_* function is
// declared in exactly one of them, with its contract, and every translation unit that defines or
// calls one includes that header (a definition that disagrees does not compile):
//   mp4x/ops.h      the kernels of libmp4x_hip.so (this file) + the shared enums and codes
//   mp4x/runtime.h  the device runtime of libmp4x_hip.so (csrc/runtime/*.hip)
//   mp4x/host.h     libmp4x_host.so (csrc/host/host_ops.cpp)
// Python binds them through two ctypes tables, mp4x/ops/hip_sigs.py and mp4x/ops/host_sigs.py;
// tests/test_native_abi_cpu.py parses the headers and holds tables, headers and the libraries'
// exports to each other.  So the headers stay flat: one prototype per `;`, no macros around
// prototypes, no function-pointer parameters.
//
// The kernel entry points are stream-ordered (no host synchronisation, no allocation) so they can
// be captured in hipGraphs.  Return value: 0 on success, otherwise a hipError_t / MP4X_E* code.
#pragma once
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

// Element types: mp4x/operators.py DType (compared by tests/test_native_abi_cpu.py).
enum mp4x_dtype {
  MP4X_F64 = 0, MP4X_F32 = 1, MP4X_I64 = 2, MP4X_I32 = 3, MP4X_I16 = 4, MP4X_I8 = 5,
  MP4X_BF16 = 6, MP4X_F16 = 7, MP4X_U8 = 8,
};

// Reduction operators: mp4x/operators.py OpCode (compared by the same test).  The reference's
// table: src/main/java/com/fenbi/mp4j/operator/Operators.java:29-353.
enum mp4x_op {
  MP4X_SUM = 0, MP4X_MAX = 1, MP4X_MIN = 2, MP4X_PROD = 3,
  MP4X_BAND = 4, MP4X_BOR = 5, MP4X_BXOR = 6,
  MP4X_FMAXLOC = 7, MP4X_FMINLOC = 8,   // f64 word: f32 value in hi 32 bits, int32 loc in lo 32 bits
  MP4X_IMAXLOC = 9, MP4X_IMINLOC = 10,  // i64 word: i32 value in hi 32 bits, int32 loc in lo 32 bits
  MP4X_FIRST = 11,                      // keep the first value (K8 map merge / dedupe-by-key; sparse only)
};

enum { MP4X_E_BADARG = 1001, MP4X_E_UNSUPPORTED = 1002,
       // latency fast path (mp4x_ipc_fast_allreduce): not launched, the caller takes the full path
       MP4X_E_FAILED_EARLIER = 1003,   // an IPC collective of this engine timed out earlier
       MP4X_E_CAPTURING = 1004,        // the stream is being captured into a hipGraph
       // a communicator's launch on a second stream inside ONE graph capture (the stream-order
       // guard cannot join a capture's forked streams: csrc/runtime/order.hip)
       MP4X_E_STREAM_SWITCH = 1005 };

#define MP4X_MAX_NIN 8

// ---------------------------------------------------------------- K1 / K1b / K2
// out[i] = op(...op(op(in[0][i], in[1][i]), in[2][i])..., in[nin-1][i])  for i < n.
// `out` may alias in[0] (the usual in-place accumulate).  nin in [1, MP4X_MAX_NIN]
// per launch; larger fan-in is chained by the caller.  16-bit floats accumulate in f32
// across the whole fan-in and round once.
int mp4x_reduce(int dtype, int op, void* out, const void* const* ins, int nin, int64_t n, void* stream);

// Same, but every input is the same buffer at a different element offset:
// in[k] = base + k * stride_elems.  Used after an all-to-all (p received chunks laid
// out contiguously) without building a pointer array.
int mp4x_reduce_strided(int dtype, int op, void* out, const void* base, int64_t stride_elems, int nin,
                        int64_t n, void* stream);

// out[i] = in[i] * scale (f32 / f64 / bf16 / f16), e.g. gradient averaging after a SUM.
int mp4x_scale(int dtype, void* out, const void* in, double scale, int64_t n, void* stream);

// ---------------------------------------------------------------- K3 segment copy
// Copy nseg byte segments in ONE launch: dst + dst_off[s] <- src + src_off[s], len[s] bytes.
// The three int64 tables live in DEVICE memory (3 * nseg entries: dst_off | src_off | len).
int mp4x_segment_copy(void* dst, const void* src, const int64_t* dev_table, int nseg, int64_t max_len,
                      void* stream);

// Row gather: out[i, :] = in[idx[i], :] for rows of `row_bytes` bytes.
int mp4x_gather_rows(void* out, const void* in, const int64_t* idx, int64_t nrows, int64_t row_bytes,
                     void* stream);

// Sparse staging: keys[n] (int64) + vals[n][row_bytes] (row_bytes a multiple of 16, 16-byte
// aligned; NULL when row_bytes == 0) -> dst_vals[n][row_bytes] + dst_keys16[n][16] (the key in
// the low 8 bytes of a 16-byte vector); keys_from16 reads such vectors back into int64 keys.
int mp4x_stage_split(const int64_t* keys, const void* vals, int64_t n, int64_t row_bytes, void* dst_vals,
                     void* dst_keys16, void* stream);
int mp4x_keys_from16(const void* keys16, int64_t n, int64_t* keys, void* stream);

// ---------------------------------------------------------------- K6 codec (fp8 e4m3, OCP)
// Block-scaled quantisation: scale[b] = amax(block b) / 448, q = fp8(x / scale).
// block must be 256 (one wave, 4 elements per lane).  n must be a multiple of 4.
int mp4x_quant_fp8(int dtype_in, const void* in, int64_t n, uint8_t* q, float* scales, void* stream);
// The same quantiser with error feedback (k_quant_ef): per element x = (float)in + resid (one f32
// add), (code, scale) = the quantisation of x exactly as above, resid = fma(-decode(code), scale, x),
// stored as 0 where that is not finite (a NaN input resets its own element, a block with an
// infinity the whole block).  resid: f32[n], read and written in place, 16-byte aligned, nothing at
// or past n touched; in is not written; q / scales: whole blocks, as above.  MP4X_E_BADARG (nothing
// launched) for n % 4 != 0, a NULL pointer, or in / resid off the 16-byte grid.
int mp4x_quant_fp8_ef(int dtype_in, const void* in, int64_t n, float* resid, uint8_t* q, float* scales, void* stream);
// out = dequant(q[0]) + ... + dequant(q[nin-1])  (f32 accumulate), optionally + out (accumulate=1).
// If q_out != NULL the f32 result is also re-quantised into (q_out, s_out).
int mp4x_dequant_reduce_fp8(int dtype_out, void* out, const uint8_t* const* qs, const float* const* scales,
                            int nin, int64_t n, int accumulate, uint8_t* q_out, float* s_out, void* stream);

// K6b lossless zero suppression.  table (device int64): elem_start[nchunk], elem_len[nchunk],
// blk_start[nchunk + 1] in 256-element blocks.  Encode: masks[4 * nblk], counts[nblk],
// offs[nblk + 1] (offs[nblk] = total non-zero words), vals (worst case n words).  Decode:
// the same masks / counts / vals (chunks concatenated) expanded into out per table.
size_t mp4x_zs_temp_bytes(int64_t nblk);
int mp4x_zs_encode(int elem_bytes, const void* in, const int64_t* table, int nchunk, int64_t nblk, uint64_t* masks,
                   int32_t* counts, int64_t* offs, void* vals, void* temp, size_t temp_bytes, void* stream);
int mp4x_zs_decode(int elem_bytes, const uint64_t* masks, const int32_t* counts, const void* vals,
                   const int64_t* table, int nchunk, int64_t nblk, void* out, int64_t* offs, void* temp,
                   size_t temp_bytes, void* stream);

// ---------------------------------------------------------------- K4 / K5 / K7 sparse
// Owner of each key: dest[i] = (uint64)key[i] % p.  hist[p] += counts (hist zeroed by caller).
int mp4x_key_owner(const int64_t* keys, int64_t n, int p, int32_t* dest, int32_t* hist, void* stream);
// Stable radix sort of (key, idx) pairs on bits [begin_bit, end_bit).  algo (int64 keys): 0 =
// rocPRIM's own choice, 1 = onesweep (one pass per 8 bits of [begin_bit, end_bit)).
size_t mp4x_sort_pairs_temp_bytes(int64_t n, int key_is_i32);
int mp4x_sort_pairs_i64(const int64_t* keys_in, int64_t* keys_out, const int64_t* idx_in, int64_t* idx_out,
                        int64_t n, int begin_bit, int end_bit, int algo, void* temp, size_t temp_bytes,
                        void* stream);
int mp4x_sort_pairs_i32key(const int32_t* keys_in, int32_t* keys_out, const int64_t* idx_in, int64_t* idx_out,
                           int64_t n, int begin_bit, int end_bit, void* temp, size_t temp_bytes, void* stream);
// Fused stable partition by owner ((uint64)key % p, p <= 2048): out_keys / out_vals (rows of
// row_bytes, 16-B aligned; vals may be NULL) in owner-major, input-stable order; out_perm
// (optional) = source row of every slot; counts[p] = rows per owner; range[2] (optional) = the
// smallest and largest key (0, 0 when n == 0).  Deterministic.
size_t mp4x_partition_pack_scratch_bytes(int64_t n, int p);
int mp4x_partition_pack(const int64_t* keys, const void* vals, int64_t n, int64_t row_bytes, int p,
                        int64_t* out_keys, void* out_vals, int64_t* out_perm, int64_t* counts, int64_t* range,
                        void* scratch, size_t scratch_bytes, void* stream);
// The two halves of mp4x_partition_pack (the same scratch between them): count -> counts[p],
// range[2]; scatter -> out_keys (key_stride 1: int64[n]; 2: the key half of 16-byte vectors),
// out_vals, out_perm.
int mp4x_partition_pack_count(const int64_t* keys, int64_t n, int p, int64_t* counts, int64_t* range, void* scratch,
                              size_t scratch_bytes, void* stream);
int mp4x_partition_pack_scatter(const int64_t* keys, const void* vals, int64_t n, int64_t row_bytes, int p,
                                int64_t* out_keys, int key_stride, void* out_vals, int64_t* out_perm, void* scratch,
                                size_t scratch_bytes, void* stream);
// Run-length encode a SORTED key array: starts[u] = first index of run u, *nruns (device int64).
size_t mp4x_rle_temp_bytes(int64_t n);
int mp4x_run_starts(const int64_t* sorted_keys, int64_t n, int64_t* starts, int64_t* nruns_dev,
                    int32_t* flags_scratch, void* temp, size_t temp_bytes, void* stream);
// Reduce-by-key over runs: for run u (rows perm[starts[u] .. starts[u+1])), out_vals[u, :] =
// op over those rows of `vals` (row length dim, dtype), in run order; out_keys[u] = key;
// out_count[u] = run length.  nruns is read from device memory.
int mp4x_segment_reduce_rows(int dtype, int op, const int64_t* sorted_keys, const int64_t* perm,
                             const int64_t* starts, const int64_t* nruns_dev, int64_t n, int64_t max_runs,
                             const void* vals, int64_t dim, int64_t* out_keys, void* out_vals, int32_t* out_count,
                             void* stream);

// K5h reduce-by-key without a sort (hash table).  supported: does the hash path serve
// (dtype, op)?  1 / 0 (every reduction of the segmented reduce except the FIRST rule, which needs
// the rank order of arbitrarily long runs).  keys[n], vals[n][dim] -> out_keys[m] (table order),
// out_vals[m][dim], out_count[m] (optional); m_flag[0] = m, written on the device (stream-ordered;
// m_flag[1] is zeroed).  out_* must hold n rows; scratch: 256-byte aligned, scratch_bytes(n).
size_t mp4x_hash_rbk_scratch_bytes(int64_t n);
int mp4x_hash_rbk_supported(int dtype, int op);
int mp4x_hash_reduce_by_key(int dtype, int op, const int64_t* keys, int64_t n, const void* vals, int64_t dim,
                            void* scratch, size_t scratch_bytes, int64_t* out_keys, void* out_vals,
                            int32_t* out_count, int64_t* m_flag, void* stream);
// K5c: the hash reduce-by-key with an output that is a function of the input alone (the same
// arguments and refusals as mp4x_hash_reduce_by_key; n == 0 gives m = 0).  out_keys[m]: the occupied
// slots, in slot order, of the canonical table (table_slots(n) slots, splitmix64 homes, the distinct
// keys other than -1 inserted in ascending unsigned order by plain linear probing:
// csrc/kernels/sparse_hash_map.hpp), then the run of rows keyed -1, if any.  out_vals[u] combines the
// run's rows in ascending input index whatever its length: the sort path's values bit for bit.
// m_flag[0] = m; m_flag[1] != 0 when a lane passed a loop bound (then nothing else is meaningful:
// use the sort path).  No allocation, no host read.
size_t mp4x_hash_rbk_canonical_scratch_bytes(int64_t n);
int mp4x_hash_reduce_by_key_canonical(int dtype, int op, const int64_t* keys, int64_t n, const void* vals, int64_t dim,
                                      void* scratch, size_t scratch_bytes, int64_t* out_keys, void* out_vals,
                                      int32_t* out_count, int64_t* m_flag, void* stream);
// K5d: keys[n] with k / stride - base in [0, T) (e.g. an owner's share of dense ids, stride = p),
// vals[n][dim] (or NULL: keys only) -> out_keys[m] ascending, out_vals[m][dim] (rows combined in
// input order: the sort path's result bit for bit), out_count[m] (optional); m_flag[0] = m,
// m_flag[1] != 0 when the keys were not dense after all (then nothing else is meaningful: use the
// sort path).
size_t mp4x_dense_rbk_scratch_bytes(int64_t n, int64_t T);
int mp4x_dense_reduce_by_key(int dtype, int op, const int64_t* keys, int64_t n, const void* vals, int64_t dim,
                             int64_t base, int64_t stride, int64_t T, void* scratch, size_t scratch_bytes,
                             int64_t* out_keys, void* out_vals, int32_t* out_count, int64_t* m_flag, void* stream);

// ---------------------------------------------------------------- K9 expert-parallel token routing
// Assignments are flattened token-major (a = t * K + k, n = T * K <= INT32_MAX / 2); the bucket of
// an assignment is its expert id (int32 or int64 by ids_are_i64), 0 <= id < nb <= 2048.  A negative
// id and an id >= nb are placed nowhere.  dtype: f32 / bf16 / f16 (else MP4X_E_UNSUPPORTED); a bad
// pointer, alignment or size is MP4X_E_BADARG before any launch.  Deterministic: no global atomics.
// Route in two halves with the same scratch (256-byte aligned, scratch_bytes(n, nb)) between them:
// count -> counts[nb + 2] = assignments per expert | negative ids | ids >= nb (zeros when n == 0).
size_t mp4x_moe_route_scratch_bytes(int64_t n, int nb);
int mp4x_moe_route_count(const void* ids, int ids_are_i64, int64_t n, int nb, int64_t* counts, void* scratch,
                         size_t scratch_bytes, void* stream);
// scatter -> slots[a] = the position of assignment a in the stable sort by id (-1: placed nowhere);
// out_rows[slots[a]] = x[a / K] (rows of row_bytes, whole 16-byte vectors, 16-byte aligned), or with
// row_scale (f32[n]) round_to_dtype(row_scale[a] * f32(x[a / K])): one multiply, one rounding.
int mp4x_moe_route_scatter(int dtype, const void* ids, int ids_are_i64, const void* x, const float* row_scale,
                           int64_t n, int K, int64_t row_bytes, int nb, void* out_rows, int64_t* slots,
                           void* scratch, size_t scratch_bytes, void* stream);
// The scatter under an expert capacity.  clip (int64[2 * nb], 8-byte aligned, device memory):
// clip[e] = keep[e], the rows of expert e this rank may send; clip[nb + e] = kept_base[e], the
// exclusive prefix of keep over the experts.  Assignment a with expert e, the pe-th of this rank's
// assignments with that expert (in a order), gets slots[a] = pe < keep[e] ? kept_base[e] + pe : -1:
// the stable sort of the kept assignments.  A clipped row is neither read nor written; out_rows
// holds sum(keep) rows.  keep[e] >= the count of e is the unclipped scatter bit for bit.  A null
// or misaligned clip is MP4X_E_BADARG, with everything the unclipped entry refuses; n == 0 is 0.
int mp4x_moe_route_scatter_clip(int dtype, const void* ids, int ids_are_i64, const void* x, const float* row_scale,
                                int64_t n, int K, int64_t row_bytes, int nb, void* out_rows, int64_t* slots,
                                const int64_t* clip, void* scratch, size_t scratch_bytes, void* stream);
// Combine: out[t] = round_to_dtype(acc), acc = +0.0f, then for k = 0 .. K-1 with slots[t*K+k] >= 0:
// acc = acc + w * f32(rows[slots[t*K+k]]), the product and the sum rounded separately (never an
// FMA), w = weights ? weights[t*K+k] : 1.  Rows of `width` elements, whole 16-byte vectors.
int mp4x_moe_combine(int dtype, const void* rows, const int64_t* slots, const float* weights, int64_t T, int K,
                     int64_t width, void* out, void* stream);
// The padded fixed-capacity layout (a per-source share): out_rows holds nb * cap rows, expert e owns
// the block [e * cap, (e + 1) * cap).  slots[a] = pe < cap ? e * cap + pe : -1 with pe as above; a
// negative id and an id >= nb get -1.  Every row of out_rows is written exactly once per call: row
// e * cap + pe by the scatter, the rows [min(cnt[e], cap), cap) of every block as all-zero bits by
// a fill kernel after it (no memset of the buffer).  n == 0 writes nb * cap zero rows and needs
// neither ids, x, slots nor scratch.  1 <= cap <= INT32_MAX / nb, else MP4X_E_BADARG.
int mp4x_moe_route_scatter_pad(int dtype, const void* ids, int ids_are_i64, const void* x, const float* row_scale,
                               int64_t n, int K, int64_t row_bytes, int nb, int64_t cap, void* out_rows, int64_t* slots,
                               void* scratch, size_t scratch_bytes, void* stream);
// After mp4x_moe_route_count on the same scratch (none when n == 0): kept[(e / el) * el_pad + e % el]
// = min(cnt[e], cap) for the nb experts in groups of el (nb % el == 0; el_pad >= el, the padding is
// zeroed; el_pad == el is the plain int64[nb]) and dropped[3] = assignments past their share |
// negative ids | ids >= nb.
int mp4x_moe_pad_counts(int64_t n, int nb, int64_t cap, int el, int el_pad, int64_t* kept, int64_t* dropped,
                        void* scratch, size_t scratch_bytes, void* stream);
// mp4x_moe_combine over a buffer of num_rows >= 1 rows that the slots index anywhere (the padded
// layout: slots reach nb * cap - 1, which may exceed T * K).  Rows no slot names are never read.
int mp4x_moe_combine_rows(int dtype, const void* rows, int64_t num_rows, const int64_t* slots, const float* weights,
                          int64_t T, int K, int64_t width, void* out, void* stream);

// ---------------------------------------------------------------- K10 fused top-k router gate
// logits[T][E], contiguous, f32 / bf16 / f16 (else MP4X_E_UNSUPPORTED), 16-byte aligned; 1 <= E <=
// 2048, 1 <= K <= min(E, 16), 0 <= T <= INT32_MAX / 2 / K, else MP4X_E_BADARG, as is a null or
// misaligned pointer (weights, lse, prob_sum, g_*: 4 bytes; ids: 4 or 8 by ids_are_i64; counts: 8;
// scratch: 256).  Every refusal comes before any launch.  All arithmetic is f32 on the exactly
// converted logits.  Deterministic: no floating-point atomics, no global atomics.
// Forward: ids[t][k] (int32 or int64 by ids_are_i64), k = 0 .. K-1, are the first K columns of row t
// in the order (logit descending, column ascending; -0 == +0; -inf last), always distinct and inside
// [0, E) whatever the bits of the row are; lse[t] = m + log(sum_j exp(l_j - m)), m the row maximum;
// weights[t][k] = p[ids[t][k]], p_j = exp(l_j - m) / sum, divided by the sum of the K chosen p (added
// in k order) when renormalize != 0.  prob_sum (f32[E]) and counts (int64[E]), both or neither:
// prob_sum[e] = sum_t p[t][e] in a fixed order, counts[e] = the number of ids equal to e; they need
// scratch of mp4x_moe_gate_scratch_bytes(dtype, T, E) bytes (0 for arguments the forward refuses),
// which is not read without them.  T == 0 launches nothing, or with the statistics writes their zeros.
size_t mp4x_moe_gate_scratch_bytes(int dtype, int64_t T, int E);
int mp4x_moe_gate_topk(int dtype, const void* logits, int64_t T, int E, int K, int renormalize, float* weights,
                       void* ids, int ids_are_i64, float* lse, float* prob_sum, int64_t* counts, void* scratch,
                       size_t scratch_bytes, void* stream);
// Backward from the saved logits, lse and ids (nothing else of size [T][E] is kept): with p_j =
// exp(l_j - lse[t]) and s = the sum of the K chosen p in k order,
//   gq_k = g_weights[t][k], or (g_weights[t][k] - sum_k' g_weights[t][k'] * p_k' / s) / s when renormalize,
//   gp_j = g_prob_sum[j] + sum_k [ids[t][k] == j] gq_k,  dot = sum_j gp_j * p_j,
//   g_logits[t][j] = round_to_dtype(p_j * (gp_j - dot) + g_lse[t] * p_j).
// g_weights (f32[T][K]), g_lse (f32[T]) and g_prob_sum (f32[E]) may each be NULL: zeros.  g_logits has
// the logits' dtype and alignment.  An id outside [0, E) takes no part (never an address).  T == 0 is 0.
int mp4x_moe_gate_backward(int dtype, const void* logits, const float* lse, const void* ids, int ids_are_i64, int64_t T,
                           int E, int K, int renormalize, const float* g_weights, const float* g_lse,
                           const float* g_prob_sum, void* g_logits, void* stream);

// ---------------------------------------------------------------- K13 group-limited router gate
// K10's gate with a choice of score, a selection bias, group-limited selection and a scaling factor.
// logits, T, E, K, weights, ids, prob_sum, counts, scratch and their refusals are K10's.  score: 0 =
// softmax (s = K10's p; lse is written and must not be NULL), 1 = sigmoid (s_j = 1 / (1 + exp(-l_j));
// lse is not touched and may be NULL); any other value is MP4X_E_UNSUPPORTED.  bias: f32[E] or NULL.
// 1 <= n_group <= 32 with E % n_group == 0 (groups of n = E / n_group contiguous columns), 1 <=
// topk_group <= n_group, K <= topk_group * n, scale finite and > 0, else MP4X_E_BADARG; bias,
// group_ids and lse are 4-byte aligned.  Every refusal comes before any launch.
// Selection score c_j = s_j + bias[j] (one rounding; s_j without a bias), -inf where l_j = -inf.  A
// group's score is the sum (one f32 addition) of its two largest c, or its largest alone when the
// second is -inf.  The chosen groups are the first topk_group in (score descending, group ascending)
// and go to group_ids[t][0 .. topk_group) (int32, optional) in that order.  ids[t][k] are the first K
// columns of the chosen groups in (key descending, column ascending): the key is the logit in K10's
// order without a bias, c with one.  For any bits the ids are distinct, inside [0, E) and inside the
// chosen groups, which are distinct and inside [0, n_group).  weights[t][k] = s[ids[t][k]], divided
// by their sum in k order when renormalize != 0, then multiplied by scale.  prob_sum[e] = sum_t
// s[t][e] and counts[e] in K10's fixed order.  T == 0 launches nothing, or with the statistics writes
// their zeros.
size_t mp4x_moe_gate_group_scratch_bytes(int dtype, int64_t T, int E);
int mp4x_moe_gate_group_topk(int dtype, const void* logits, const float* bias, int64_t T, int E, int K, int n_group,
                             int topk_group, int score, int renormalize, float scale, float* weights, void* ids,
                             int ids_are_i64, int32_t* group_ids, float* lse, float* prob_sum, int64_t* counts,
                             void* scratch, size_t scratch_bytes, void* stream);
// Backward from the saved logits, ids and (softmax) lse; the bias has no gradient.  With q_k the
// score of column ids[t][k] and S their sum in k order:
//   gq_k = scale * g_weights[t][k], or scale * ((g_weights[t][k] - sum_i g_weights[t][i] * (q_i / S)) / S)
//   when renormalize;  gp_j = g_prob_sum[j] + sum_k [ids[t][k] == j] gq_k;
//   softmax: g_logits[t][j] = round_to_dtype(p_j * (gp_j - sum_i gp_i p_i) + g_lse[t] * p_j), p_j = exp(l_j - lse[t]);
//   sigmoid: g_logits[t][j] = round_to_dtype(d_j * gp_j), d_j = sigmoid(l_j) * sigmoid(-l_j), each factor
//   by the forward's formula; lse and g_lse are not read.
// NULL gradients are zeros; an id outside [0, E) takes no part (never an address).  T == 0 is 0.
int mp4x_moe_gate_group_backward(int dtype, const void* logits, const float* lse, const void* ids, int ids_are_i64,
                                 int64_t T, int E, int K, int score, int renormalize, float scale,
                                 const float* g_weights, const float* g_lse, const float* g_prob_sum, void* g_logits,
                                 void* stream);

// ---------------------------------------------------------------- K11 fused combine backward
// Both gradients of mp4x_moe_combine from one pass over its output gradient g[T][width]: rows
// [num_rows][width] are the rows the combine read (slot order), g_rows [num_rows][width] their
// gradient; all three f32 / bf16 / f16 (else MP4X_E_UNSUPPORTED), rows of whole 16-byte vectors,
// 16-byte aligned.  slots int64[T*K], weights and g_weights f32[T*K]; 1 <= K <= 16, 0 <= T <=
// INT32_MAX / 2 / K, num_rows >= 1.  A null or misaligned pointer, a bad size, K > 16 and a g_rows
// that overlaps rows or g are MP4X_E_BADARG before any launch; T == 0 launches nothing.
// Per assignment a = t*K + k with s = slots[a] >= 0:
//   g_rows[s]    = round_to_dtype(weights[a] * f32(g[t])): one multiply, one rounding, bit for bit
//                  what mp4x_moe_route_scatter writes with row_scale;
//   g_weights[a] = sum_h f32(g[t][h]) * f32(rows[s][h]) in f32 (contraction to FMA allowed), in an
//                  order fixed by (dtype, width) alone;
// with s < 0 no row is read or written and g_weights[a] = +0.0f.  Every slot value appears at most
// once; a row of g_rows no slot names is not touched.  Deterministic: no atomics.
int mp4x_moe_combine_backward(int dtype, const void* g, const void* rows, int64_t num_rows, const int64_t* slots,
                              const float* weights, int64_t T, int K, int64_t width, void* g_rows, float* g_weights,
                              void* stream);
// The same into the padded layout after mp4x_moe_route_count / mp4x_moe_route_scatter_pad on the
// same scratch (n = T*K assignments, nb experts, share cap; the slots are that scatter's): num_rows
// = nb * cap, and the pad rows [min(cnt[e], cap), cap) of every expert block are then written as
// all-zero bits by the fill kernel, so every row of g_rows is written exactly once, as
// mp4x_moe_route_scatter_pad with row_scale leaves it.  n == 0 writes nb * cap zero rows and needs
// neither g, rows, slots, weights, g_weights nor scratch.
int mp4x_moe_combine_backward_pad(int dtype, const void* g, const void* rows, const int64_t* slots, const float* weights,
                                  int64_t T, int K, int64_t width, int64_t n, int nb, int64_t cap, void* scratch,
                                  size_t scratch_bytes, void* g_rows, float* g_weights, void* stream);

// ---------------------------------------------------------------- K15 per-expert top-S select (drop by gate weight)
// After mp4x_moe_route_count on the same ids (route_scratch is its scratch, read only): out_ids[a] =
// ids[a] for the limit[e] assignments of every expert e = ids[a] in [0, nb) with the largest key
// (gate_key(priority[a]), -a), compared lexicographically: the order-preserving map of the f32 bits
// (unsigned order == float order, -0 folded onto +0, a positive NaN above +inf, a negative one below
// -inf), ties to the lower a; -1 for the other assignments of e.  A negative id and an id >= nb pass
// through.  limit[e] = limit_vec[e] (int64[nb], device memory, 8-byte aligned; a negative entry counts
// as 0) or, with limit_vec NULL, the scalar limit >= 0.  out_ids has the ids' width and alignment and
// is not ids.  masked[0] = the assignments turned into -1.  Expert e keeps exactly min(cnt[e],
// limit[e]); with a constant priority they are its first ones.  An expert within its limit costs no
// selection work; the others an 8-pass radix select over their contiguous words: work bounded by a
// constant * n however the ids are distributed.  Integer arithmetic only, no global atomics, no host
// read: deterministic and recordable in a graph.  scratch: 256-byte aligned,
// mp4x_moe_priority_scratch_bytes(n, nb) bytes (0 for arguments the call refuses).  nb, n, pointers
// and alignment as in mp4x_moe_route_count, else MP4X_E_BADARG before any launch; n == 0 writes
// masked = 0 and needs nothing else.
size_t mp4x_moe_priority_scratch_bytes(int64_t n, int nb);
int mp4x_moe_priority_mask(const void* ids, int ids_are_i64, const float* priority, int64_t n, int nb, int64_t limit,
                           const int64_t* limit_vec, const void* route_scratch, size_t route_scratch_bytes,
                           void* out_ids, int64_t* masked, void* scratch, size_t scratch_bytes, void* stream);

// ---------------------------------------------------------------- errors
// Reads and clears this thread's last HIP error.  mp4x reports its own failures through return
// codes; a failed HIP call must not stay "last error" for PyTorch's next kernel-launch check to
// report as its own (native.check() and the best-effort release paths call this).
int mp4x_clear_error(void);

// ---------------------------------------------------------------- test / A-B hooks
// Process-wide switches of the kernel-variant sweeps (tools/bench_kernels.py, bench/, the codec
// tests); never set by a job.  k1_variant: the K1 kernel form (default 2: tile + nontemporal);
// k1_grid: its grid cap in blocks (0: one tile per block).  dq_unroll: quant blocks per wave iteration
// of the dequant-reduce (0: by fan-in); codec_grid: 1 = the codec launches its whole grid (the
// default), 0 = the capped grid-stride form.  zs_set_twopass: 1 = mask + scan + compact (two reads
// of the input, the default), 0 = the single-pass encode.
void mp4x_set_k1_variant(int v);
void mp4x_set_k1_grid(int64_t cap);
void mp4x_set_dq_unroll(int du);
void mp4x_set_codec_grid(int full);
int mp4x_zs_set_twopass(int on);

#ifdef __cplusplus
}
#endif
