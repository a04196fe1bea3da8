"""Can a rank import a PEER's memAlloc chunk?  memAlloc (parallel/vmm.py) hands every chunk to the
peers as a dmabuf fd and each peer turns it into an allocation handle with
``hipMemImportFromShareableHandle``.  Some platforms (a virtualised GPU whose kernel driver is a
proxy) refuse exactly that call for a chunk another process created — ``invalid argument``, while
the same fd imports fine in the process that exported it — and nothing else maps several chunks
back to back in a peer.  There memAlloc falls back to plain tensors (process_comm.memAlloc), and
the tests whose subject is the peer-mapped allocation itself have nothing to check.

:func:`require_peer_vmm_import` asks once per session, with 2 ranks that do nothing but create one
2 MiB chunk each, exchange the fds and import the other's; it skips the calling test only for that
one refusal (any other error is raised).
"""
import functools

import pytest

HIP_ERROR_INVALID_VALUE = 1
REASON = "hipMemImportFromShareableHandle of a peer process's dmabuf fd is not supported here"


def _peer_import_fn(comm):
    import os

    import torch  # noqa: F401 — before the native library (shared HIP runtime)
    from mp4x.exceptions import NativeError
    from mp4x.ops import native
    from mp4x.parallel import vmm
    r, p = comm.getRank(), comm.getSlaveNum()
    lib = native.hip()
    pool = vmm.ChunkPool(lib)
    (c,) = pool.take([2 << 20])
    got = vmm.exchange_fds(comm.server, r, p, [c.fd])
    code = 0
    try:
        pool.import_fd(1 - r, c.id, got[1 - r][0])
    except NativeError as e:
        if e.code != HIP_ERROR_INVALID_VALUE:
            raise
        code = e.code
    finally:
        for fl in got.values():
            for fd in fl:
                os.close(fd)
    for h in pool.peer.values():              # importers release first, the owners after a barrier
        native.check(lib.mp4x_vmm_chunk_release(h), "vmm_chunk_release")
    pool.peer = {}
    comm.server.call("barrier", r)
    pool.release_all()
    return code


@functools.lru_cache(maxsize=None)
def peer_vmm_import_supported() -> bool:
    from spawn_ranks import run_spawn
    out = run_spawn(2, _peer_import_fn, timeout=120)
    return not any(out.values())


def require_peer_vmm_import() -> None:
    if not peer_vmm_import_supported():
        pytest.skip(REASON)
