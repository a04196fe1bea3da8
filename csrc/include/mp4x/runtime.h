// mp4x native C API: the device runtime of libmp4x_hip.so (csrc/runtime/*.hip) — the custom xGMI
// collectives over IPC-mapped peer buffers, their memory and signal blocks, the stream-order
// guard, the VMM allocations, the topology and coherence probes.  See mp4x/ops.h for the rules
// the three ABI headers follow; the protocol itself is described in csrc/runtime/ipc_common.hpp.
//
// Plain C, no HIP includes: streams, events and device pointers cross as void*.
// Return value unless stated otherwise: 0 on success, else a hipError_t / MP4X_E_* code.
// Common arguments of the collectives:
//   data_ptrs / signal_ptrs  p entries (own rank included, peers as mapped by
//                            mp4x_ipc_open_handle); data buffers are 16-byte aligned
//   epoch / epoch_dev        epoch_dev == NULL: `epoch` (the host counter) is used; != NULL: the
//                            graph-capturable form, the kernel reads the epoch from device memory
//                            (bump it with mp4x_ipc_bump_epoch first) and keeps epoch's tag bits
//   blocks                   workgroups to launch; <= 0: chosen from the message size
//   op                       any operator of the reference table valid for dtype
//                            (MP4X_E_UNSUPPORTED otherwise)
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "mp4x/ops.h"

#ifdef __cplusplus
extern "C" {
#endif

// ---------------------------------------------------------------- memory, handles, signal blocks
// sizeof(Signal): one rank's signal block.
size_t mp4x_ipc_signal_bytes(void);
// Fine-grained, uncached device allocation (signal blocks and IPC data buffers), zeroed.
int mp4x_ipc_alloc(size_t bytes, void** ptr);
int mp4x_ipc_free(void* ptr);
// Staging data buffer of an IPC instance, zeroed: coarse = 0 -> fine-grained uncached (the
// default: peers' reads never meet a stale L2 line); 1 -> plain coarse-grained hipMalloc memory,
// L2-cached on its home GPU, kept coherent by the kernels' system-scope release / acquire at
// every barrier (the zero-copy protocol's argument).  MP4X_IPC_DATA_MEM selects it (A/B).
int mp4x_ipc_alloc_data(size_t bytes, int coarse, void** ptr);
// Plain (coarse-grained) device allocation, the kind the PyTorch caching allocator makes: the
// self-test of the zero-copy protocol runs on memory like the caller tensors it will map.
int mp4x_dev_alloc(size_t bytes, void** ptr);
// Pinned host word the kernels can write (mapped, coherent): *host_ptr for the CPU, *dev_ptr for
// the kernels.  Zeroed.
int mp4x_host_word_alloc(void** host_ptr, void** dev_ptr);
int mp4x_host_word_free(void* host_ptr);
// Register the host-visible error word of a signal block (device address from
// mp4x_host_word_alloc; NULL to detach).
int mp4x_ipc_set_host_error(void* signal, void* dev_word);
// Barrier spin bound of the kernels that use `signal` (this rank's own Signal block), in seconds.
// Stream-ordered on `stream` (kernels queued before it keep the previous bound), then synchronised.
int mp4x_ipc_set_spin(void* signal, double seconds, void* stream);
// The signal block's error word read on `stream` (a private non-blocking stream, so a poll from
// the collective watchdog thread never serialises with the caller's streams); clear != 0 resets
// it after the read, so one timed-out barrier is reported once instead of poisoning every later
// check.
int mp4x_ipc_error_word(void* signal, uint32_t* err, int clear, void* stream);
// Bump the device epoch counter of a graph-capturable instance (stream-ordered: the next IPC
// kernel on `stream` reads the new epoch).
int mp4x_ipc_bump_epoch(uint32_t* epoch_dev, void* stream);
// PCI bus id of the current device: ranks compare them to detect a GPU shared by several ranks
// (single-GPU rehearsal), where the per-block barriers need every rank's blocks co-resident and
// the block count must shrink accordingly.
int mp4x_device_pci_id(char* buf, int len);
// Base and size of the allocation that contains `ptr` (IPC handles name whole allocations: a
// caller tensor inside a caching-allocator segment is exported as (segment handle, offset)).
int mp4x_mem_range(void* ptr, void** base, size_t* size);
// hipIpcMemHandle_t as mp4x_ipc_handle_size() opaque bytes: export `ptr`'s allocation / map a
// peer's (lazy peer access) / unmap it.
int mp4x_ipc_handle_size(void);
int mp4x_ipc_get_handle(void* ptr, void* handle_out);
int mp4x_ipc_open_handle(const void* handle, void** ptr);
int mp4x_ipc_close_handle(void* ptr);
// Device-to-device copy / byte fill on `stream`.
int mp4x_memcpy_async(void* dst, const void* src, size_t bytes, void* stream);
int mp4x_memset_async(void* dst, int value, size_t bytes, void* stream);

// ---------------------------------------------------------------- allreduce
// One-shot (algo 0) / two-shot (algo 1) allreduce.  nbytes must be a multiple of 16.
// src != NULL: this rank's input (16-byte aligned) is copied into its own buffer INSIDE the
// kernel (fused copy-in: one launch per call); NULL: already staged, or zero-copy (the data
// pointers are the registered caller tensors and out == data_ptrs[rank]).  scale != 1: the
// reduced value is multiplied by it before it is stored (fused average; float dtypes only).
// slot_base / slot_vecs (16-byte vectors): the latency tier's two staging slots at vector offset
// slot_base + (epoch & 1) * slot_vecs, with no end barrier; 0 / 0 = the single-buffer form with
// its end barrier.  A slotted call needs src (the staging target depends on the device-side
// epoch) and nbytes <= a slot.
int mp4x_ipc_allreduce(int algo, int dtype, int op, void* const* data_ptrs, void* const* signal_ptrs, int rank,
                       int p, int64_t nbytes, const void* src, void* out, uint32_t epoch, int blocks,
                       const uint32_t* epoch_dev, float scale, void* stream, int64_t slot_base, int64_t slot_vecs);
// Zero-copy PUSH two-shot: data_ptrs = every rank's registered tensor (this rank's own included;
// the result replaces it), scratch_ptrs = every rank's receive scratch of at least
// (p - 1) * ceil(nbytes / 16 / p) 16-byte vectors.
int mp4x_ipc_allreduce_push(int dtype, int op, void* const* data_ptrs, void* const* scratch_ptrs,
                            void* const* signal_ptrs, int rank, int p, int64_t nbytes, uint32_t epoch, int blocks,
                            const uint32_t* epoch_dev, float scale, void* stream);
// Fused fp8 two-shot allreduce of one piece.  Every rank has already quantised its input into its
// own buffer (q bytes at 0, f32 scales at `soff`, p * cb quant blocks, blocks past the input
// zeroed); `out` (dtype = f32 / bf16 / f16, 16-B aligned) receives n elements.
int mp4x_ipc_fp8_allreduce(int dtype, void* const* data_ptrs, void* const* signal_ptrs, int rank, int p, int64_t cb,
                           int64_t soff, void* out, int64_t n, uint32_t epoch, int blocks,
                           const uint32_t* epoch_dev, float scale, void* stream);
// The halves of the fp8 two-shot as collectives over ragged per-rank segments, one piece per call
// (dtype = f32 / bf16 / f16; the quantise into the own buffer ran just before on `stream`).
// Segment bounds are elements, multiples of 4; soff (16-B aligned, past the q bytes) is where the
// f32 scales start in EVERY rank's buffer; blocks <= 0 = a grid from the largest share of any
// rank.  _check: every refusal of the call without launching; the launcher runs it first.
// Reduce-scatter: every rank quantised the piece's whole range, `nblk` quant blocks counted from
// the piece's first element; seg_lo / seg_hi[p] = every rank's segment from that element (in
// ascending order, inside the nblk blocks); `out` (16-B aligned) = the address of that element in
// this rank's tensor.  Writes seg_lo[rank] .. seg_hi[rank] only: the f32 sum in rank order of all
// p dequantised buffers, stored with one rounding.
int mp4x_ipc_fp8_reduce_scatter(int dtype, void* const* data_ptrs, void* const* signal_ptrs, int rank, int p,
                                int64_t nblk, int64_t soff, const int64_t* seg_lo, const int64_t* seg_hi, void* out,
                                uint32_t epoch, int blocks, const uint32_t* epoch_dev, void* stream);
int mp4x_ipc_fp8_reduce_scatter_check(int dtype, int rank, int p, int64_t nblk, int64_t soff, const int64_t* seg_lo,
                                      const int64_t* seg_hi, const void* out);
// All-gather: rank k quantised ITS segment on a block grid counted from the segment's start (at
// most `maxblk` blocks, the largest segment's); seg_lo / seg_hi[p] = where every rank's segment
// lands in `out` (16-B aligned; elements from it).  Every segment, the own one included, is
// dequantised into out, so all ranks hold the same bytes.
int mp4x_ipc_fp8_allgather(int dtype, void* const* data_ptrs, void* const* signal_ptrs, int rank, int p,
                           int64_t maxblk, int64_t soff, const int64_t* seg_lo, const int64_t* seg_hi, void* out,
                           uint32_t epoch, int blocks, const uint32_t* epoch_dev, void* stream);
int mp4x_ipc_fp8_allgather_check(int dtype, int rank, int p, int64_t maxblk, int64_t soff, const int64_t* seg_lo,
                                 const int64_t* seg_hi, const void* out);
// Ragged all-to-all with the fp8 codec on the links (dtype = f32 / bf16 / f16): every rank
// quantised its WHOLE send buffer, flattened, on one block grid counted from its first element
// (q bytes at 0, f32 scales at `soff` in EVERY rank's buffer; nblk_peer[k] = the quant blocks of
// rank k's send, which bound the reads).  This rank receives, from every peer k, the elements
// [elo[k], ehi[k]) of k's buffer at out[dst[k] ...] (elements, multiples of 4; the dst ranges in
// rank order without overlap; `out` 16-B aligned), dequantised with one rounding; nothing else is
// written.  `blocks` >= 1 and the same on every rank: the caller sizes it from the largest
// (sender, receiver) segment of the whole count matrix, which one rank's arguments do not show.
// _check: every refusal of the call without launching; the launcher runs it first.
int mp4x_ipc_fp8_alltoall(int dtype, void* const* data_ptrs, void* const* signal_ptrs, int rank, int p,
                          int64_t soff, const int64_t* elo, const int64_t* ehi, const int64_t* dst,
                          const int64_t* nblk_peer, void* out, uint32_t epoch, int blocks,
                          const uint32_t* epoch_dev, void* stream);
int mp4x_ipc_fp8_alltoall_check(int dtype, int rank, int p, int64_t soff, const int64_t* elo, const int64_t* ehi,
                                const int64_t* dst, const int64_t* nblk_peer, const void* out);
// Does the IPC allreduce have a kernel for (dtype, op)?  1 / 0.
int mp4x_ipc_op_supported(int dtype, int op);

// ---------------------------------------------------------------- reduce-scatter, all-gather, copy plans
// Reduce-scatter over staged buffers: out (16-B aligned) receives vectors [vec_lo, vec_hi) of the
// op-reduction of all p buffers.  Every rank stages its WHOLE range before the call.
int mp4x_ipc_reduce_scatter(int dtype, int op, void* const* data_ptrs, void* const* signal_ptrs, int rank, int p,
                            int64_t vec_lo, int64_t vec_hi, void* out, uint32_t epoch, int blocks,
                            const uint32_t* epoch_dev, void* stream);
// Reduce-scatter with fused staging: `src` (16-B aligned) holds this rank's whole range laid out
// like the buffer (vector offsets seg_lo / seg_hi per rank, relative to src and to the buffer);
// this rank's reduced segment goes straight to `out` (16-B aligned) at out[v - lo].  One launch.
// _check: every refusal of the call without launching (alignment, rank range, segment bounds, the
// (dtype, op) pair) — the latency fast path runs it before its epoch moves.
int mp4x_ipc_reduce_scatter_from(int dtype, int op, void* const* data_ptrs, void* const* signal_ptrs, int rank,
                                 int p, const int64_t* seg_lo, const int64_t* seg_hi, const void* src, void* out,
                                 uint32_t epoch, int blocks, const uint32_t* epoch_dev, void* stream);
int mp4x_ipc_reduce_scatter_from_check(int dtype, int op, int rank, int p, const int64_t* seg_lo,
                                       const int64_t* seg_hi, const void* src, const void* out);
// All-gather of ragged segments: seg_lo / seg_hi[p] (host arrays, 16-B vectors from the buffer
// base); every rank stages its own segment at its offset; out (the same layout, 16-B aligned)
// receives every peer's segment.
int mp4x_ipc_allgather(void* const* data_ptrs, void* const* signal_ptrs, int rank, int p, const int64_t* seg_lo,
                       const int64_t* seg_hi, void* out, uint32_t epoch, int blocks, const uint32_t* epoch_dev,
                       void* stream);
// Copy plan (broadcast / gather / scatter / all-gather in one kernel).  stage / pull: n x
// {src_off, dst_off, len, peer} int64 quadruples in 16-byte vectors: this rank stages `stage`
// items from src into its own buffer, then pulls `pull` items from the peers' buffers into out.
// grid_len (vectors) must be rank-independent — the largest item of any rank — so every rank
// launches the same grid; buf_vecs bounds every item.  _check: every refusal of the call without
// launching (the latency fast path runs it before its epoch moves).
int mp4x_ipc_copy_plan(void* const* data_ptrs, void* const* signal_ptrs, int rank, int p, const int64_t* stage,
                       int nstage, const int64_t* pull, int npull, const void* src, void* out, int64_t grid_len,
                       int64_t buf_vecs, uint32_t epoch, int blocks, const uint32_t* epoch_dev, void* stream);
int mp4x_ipc_copy_plan_check(int rank, int p, const int64_t* stage, int nstage, const int64_t* pull, int npull,
                             const void* src, const void* out, int64_t buf_vecs);

// ---------------------------------------------------------------- occupancy
// Blocks per CU the occupancy API admits for the kernel such a call launches: the shared-GPU
// co-residency budget (mp4x/parallel/occupancy.py).  _misc families: 0 = the ragged all-gather,
// 1 = the copy plan, 2 / 3 = the fused fp8 two-shot, wide / narrow (dtype = the output dtype),
// 4 / 5 = the fp8 reduce-scatter / all-gather halves, 6 = the fp8 ragged all-to-all.
int mp4x_ipc_occupancy_ar(int algo, int dtype, int op, int p, int* blocks_per_cu);
int mp4x_ipc_occupancy_push(int dtype, int op, int p, int* blocks_per_cu);
int mp4x_ipc_occupancy_rs(int dtype, int op, int p, int* blocks_per_cu);
int mp4x_ipc_occupancy_misc(int family, int dtype, int p, int* blocks_per_cu);

// ---------------------------------------------------------------- stream-order guard
// One communicator's collectives run in the order they were issued, whatever streams they were
// issued on (csrc/runtime/order.hip).  The state is mp4x.parallel.order.StreamOrder; opaque here.
typedef struct mp4x_stream_order mp4x_stream_order;
// Order `stream` after the communicator's previous launch: 0, MP4X_E_STREAM_SWITCH (a second
// stream inside one graph capture) or a HIP error.  o == NULL: no guard, 0.  capturing: 0 = the
// caller knows the stream is not being captured, 1 = it is, -1 = unknown (queried).  The steady
// state (same stream as the previous launch, not capturing) is one compare.
int mp4x_order_enter_ex(mp4x_stream_order* o, void* stream, int capturing);
// mp4x_order_enter_ex(o, stream, 0): the native fast paths, which checked the capture themselves.
int mp4x_order_enter(mp4x_stream_order* o, void* stream);
// Release the guard's event (the communicator is closing; its streams were drained).
int mp4x_order_release(mp4x_stream_order* o);

// ---------------------------------------------------------------- latency fast paths
// The latency tier's whole per-call host path in ONE native call, bound by address in
// csrc/pyext/launch_ext.cpp.  The Python entry looks its call shape up in the engine's memo and
// hands over the memoised launch; everything the Python path did per call happens natively:
//   * the fail-stop check: every IPC instance's pinned host error word (an earlier collective
//     that timed out fails the next call: MP4X_E_FAILED_EARLIER, the caller raises);
//   * the capture check: a stream being captured needs the device-epoch form (MP4X_E_CAPTURING);
//   * every argument refusal of the launcher (MP4X_E_BADARG / MP4X_E_UNSUPPORTED);
//   * the communicator's stream order (mp4x_order_enter);
//   * the epoch bump, in the instance's epoch box (the same word IpcAllreduce.epoch reads);
//   * the launch.
// Every refusal comes BEFORE the epoch moves (1001-1004: nothing happened, the caller may take
// the full path).  A launch that fails AFTER it (a HIP error) leaves this rank at the same epoch
// as its peers, whose kernels of this call then time out at their start barrier: that is
// consistent, so the epoch is NOT rolled back; instead the instance's own host error word gets
// code 5, and this rank's next call fails at once instead of waiting for them.
//
// The per-instance state; the ctypes mirror is mp4x.parallel.ipc.FastAr (layouts compared by
// tests/test_native_abi_cpu.py).
typedef struct FastAr {
  const uint32_t* herr[8];   // pinned host error words of the engine's instances (NULL ends the list)
  uint32_t* epoch;           // the instance's epoch box
  void* const* data_ptrs;    // every rank's staging buffer
  void* const* signal_ptrs;  // every rank's signal block
  int32_t rank, p;
  int64_t slot_base, slot_vecs;   // the double-buffered slots of the one- / two-shot (0: none)
  mp4x_stream_order* order;  // the communicator's stream-order guard (NULL: none)
  uint32_t* own_err;         // this instance's pinned host error word (launch failures: code 5)
} FastAr;
// mp4x_ipc_allreduce, in place on buf (fused copy-in, fused scale), slotted when nbytes fits a slot.
int mp4x_ipc_fast_allreduce(const FastAr* s, int algo, int dtype, int op, void* buf, int64_t nbytes, int blocks,
                            float scale, void* stream);
// mp4x_ipc_copy_plan for a memoised plan.  src_off / out_off: byte offsets of the plan's source /
// output from `base` (the caller's tensor), or -1 for none.
int mp4x_ipc_fast_plan(const FastAr* s, const int64_t* stage, int nstage, const int64_t* pull, int npull,
                       int64_t src_off, int64_t out_off, void* base, int64_t grid_len, int64_t buf_vecs, int blocks,
                       void* stream);
// mp4x_ipc_reduce_scatter_from for a memoised call.  seg_lo / seg_hi: p segment bounds in 16-byte
// vectors from the range start; src_off / out_off: byte offsets from `base`.
int mp4x_ipc_fast_rs(const FastAr* s, int dtype, int op, const int64_t* seg_lo, const int64_t* seg_hi,
                     int64_t src_off, int64_t out_off, void* base, int blocks, void* stream);

// ---------------------------------------------------------------- VMM allocations (memAlloc)
// Peer-mappable allocations of any size from the virtual memory API (csrc/runtime/vmm.hip).
// Recommended allocation granularity (bytes) of the current device for fd-exportable memory.
int mp4x_vmm_granularity(size_t* gran);
// Allocate n chunks of `chunk` bytes (granularity multiple) mapped back to back at a fresh VA
// range.  fds (n entries) get one exported POSIX fd per chunk when fds is not NULL; handles (n
// entries) get the generic allocation handles.  On failure everything created so far is released
// and the fds closed.
int mp4x_vmm_create(size_t chunk, int n, void** va_out, uint64_t* handles, int* fds);
// Import a peer's n chunk fds and map them back to back at a fresh VA range of this process,
// read/write for the current device.  The fds are NOT closed here (the caller owns them; the
// imported handles keep the memory alive).
int mp4x_vmm_import(const int* fds, size_t chunk, int n, void** va_out, uint64_t* handles);
// Unmap + release n chunks mapped at va and free the VA range (own or imported).
int mp4x_vmm_free(void* va, size_t chunk, int n, const uint64_t* handles);
// Unmap + release the chunks but keep the VA range reserved for the rest of the process: no later
// reservation lands on these addresses, and no hipMemAddressFree happens.
int mp4x_vmm_release_keep_va(void* va, size_t chunk, int n, const uint64_t* handles);
// The chunk pool (the memAlloc default).  One physical chunk of `bytes` (granularity multiple);
// fd (nullable) gets its dmabuf fd.
int mp4x_vmm_chunk_create(size_t bytes, uint64_t* handle, int* fd);
// A peer's chunk from its dmabuf fd (the fd stays the caller's).
int mp4x_vmm_chunk_import(int fd, uint64_t* handle);
int mp4x_vmm_chunk_release(uint64_t handle);
// Reserve a fresh range of sum(sizes) bytes and map n chunks back to back, read/write for the
// current device.  On failure the chunks mapped so far are unmapped and the range is left
// reserved (never freed); *va_out gets it either way (0 if the reservation failed).
int mp4x_vmm_map_chunks(const uint64_t* handles, const size_t* sizes, int n, void** va_out);
// Unmap n chunks mapped back to back at va (the range stays reserved, the chunks alive).
int mp4x_vmm_unmap_chunks(void* va, const size_t* sizes, int n);
// Turn the address hint mode on / off; returns the cursor (the next hinted address, 0 = none yet).
uint64_t mp4x_vmm_va_hint(int on);
// System-scope release on every XCD (one small kernel on `stream`): makes what earlier kernels
// wrote into coarse-grained memory visible to readers that do not go through this GPU's L2 (a
// peer over xGMI, or another mapping).
int mp4x_release_all(void* stream);

// ---------------------------------------------------------------- probes
// For every ordered pair (a, b) of the n visible devices fill row-major n*n arrays:
//   link[a*n+b]    HSA link type (4 = xGMI, 2 = PCIe; -1 = unknown / a == b)
//   hops[a*n+b]    hop count (0 on the diagonal)
//   access[a*n+b]  hipDevP2PAttrAccessSupported
//   rank[a*n+b]    hipDevP2PAttrPerformanceRank
//   atomics[a*n+b] hipDevP2PAttrNativeAtomicSupported
// Returns the number of devices written (<= cap), or -(hipError) on failure.  Touches no device
// memory; safe to call before any allocation.
int mp4x_topology(int cap, int* link, int* hops, int* access, int* rank, int* atomics);
// Cross-XCD coherence probe on caller-provided device buffers: `data` (8 * region_vecs 16-byte
// vectors, any contents), `flags` (512 u32, 128-byte aligned, zeroed by this call), `out` (34 u32,
// zeroed by this call).  mask: 1 / 2 leave the producer's release / the consumer's acquire out.
int mp4x_xcd_probe(void* data, void* flags, void* out, int64_t region_vecs, int rounds, uint32_t mask, double spin_s,
                   void* stream);

// ---------------------------------------------------------------- test / A-B hooks
// 1 in the MP4X_DEBUG build (libmp4x_hip_debug.so), else 0.
int mp4x_debug_build(void);
// The debug flags of an IPC instance's own Signal block (1 = no release, 2 = no acquire in
// block_barrier): read by the debug build only; the release kernels ignore them.
int mp4x_ipc_set_debug(void* signal, uint32_t flags);

#ifdef __cplusplus
}
#endif
