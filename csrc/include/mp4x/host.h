// mp4x native C API: libmp4x_host.so (csrc/host/host_ops.cpp) — the CPU reduction kernels, the
// shared-memory intra-node data plane and the in-process thread team.  No GPU dependency.  See
// mp4x/ops.h for the rules the three ABI headers follow; dtype / op are its mp4x_dtype / mp4x_op.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "mp4x/ops.h"

#ifdef __cplusplus
extern "C" {
#endif

// ---------------------------------------------------------------- reduction
// out[i] = op(in[0][i], ..., in[nin-1][i]) for i < n, inputs folded in order, on nthreads threads
// (<= 1, or a short n: the calling thread).  `out` may alias in[0].  0, or MP4X_E_BADARG /
// MP4X_E_UNSUPPORTED.
int mp4x_host_reduce(int dtype, int op, void* out, const void* const* ins, int nin, int64_t n, int nthreads);

// ---------------------------------------------------------------- /dev/shm data plane
// One segment shared by the p ranks of a host: a 4096-byte header, then one slot of slot_bytes per
// rank.  The collectives return 0, -1 (the barrier timed out and is aborted for everyone), -2
// (aborted), -3 (a peer process exited; aborted for everyone) or an MP4X_E_* code.
//
// Attach rank `rank` to the mapped segment at `base` (zero-filled by its creator; rank 0
// initialises the header).  timeout_s <= 0: 300 s.  Returns the handle of the other calls.
void* mp4x_shm_attach(void* base, int rank, int p, int64_t slot_bytes, int nthreads, double timeout_s);
void mp4x_shm_detach(void* h);
// After every rank attached: turn on peer-death detection in the barrier iff every peer is
// visible in this process's /proc with the start time it published (same pid namespace).
// Returns 1 when enabled, 0 when not (the barrier then relies on its timeout alone).
int mp4x_shm_watch_peers(void* h);
int mp4x_shm_barrier(void* h);
// In-place allreduce of buf[0, n) (elements), in pieces of one slot each.
int mp4x_shm_allreduce(void* h, int dtype, int op, void* buf, int64_t n);
// Ragged reduce-scatter: rank r ends with the reduction of every rank's [froms[r], tos[r]).
int mp4x_shm_reduce_scatter(void* h, int dtype, int op, void* buf, const int64_t* froms, const int64_t* tos);
// Ragged allgather of es-byte elements: every rank ends with every rank's [froms[j], tos[j]).
int mp4x_shm_allgather(void* h, int es, void* buf, const int64_t* froms, const int64_t* tos);
// Root's [frm, to) (es-byte elements) copied into every other rank's buffer.
int mp4x_shm_broadcast(void* h, int es, void* buf, int64_t frm, int64_t to, int root);

// ---------------------------------------------------------------- thread team
// The thread level of ThreadCommSlave for host arrays, below the GIL: n threads, each makes ONE
// call per phase with its thread id.  timeout_s <= 0: no timeout.  NULL when n < 1.  Every
// collective returns 0, -1 (timed out; the team is then aborted for everyone), -2 (aborted) or
// MP4X_E_UNSUPPORTED (dtype).
void* mp4x_team_create(int n, double timeout_s);
void mp4x_team_destroy(void* h);
void mp4x_team_abort(void* h);
int mp4x_team_aborted(void* h);
int mp4x_team_barrier(void* h, int tid);
// [f, t) of every thread's buffer reduced into the root thread's buffer (the root's value first,
// then the others in thread order), then a barrier.
int mp4x_team_reduce(void* h, int tid, void* buf, int64_t f, int64_t t, int dtype, int op, int root);
// Root's [f, t) copied into every other thread's buffer: publish, barrier, copy, barrier.
int mp4x_team_bcast(void* h, int tid, void* buf, int64_t f, int64_t t, int elem_bytes, int root);
// Fused thread-level allreduce: publish, barrier, each thread reduces its chunk of every buffer
// and writes the result into every buffer's chunk, barrier.  Two meetings.
int mp4x_team_allreduce(void* h, int tid, void* buf, int64_t f, int64_t t, int dtype, int op);

#ifdef __cplusplus
}
#endif
