"""ctypes binding of librecsys_hip.so (include/recsys_hip.h).

This is the only place Python touches the C-ABI. There is no CPU fallback: if the library is
missing, or no gfx950 device is visible when a kernel is called, the call raises.
"""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

import torch

from ._header import read_header

_PKG = Path(__file__).resolve().parent
LIB_PATH = _PKG / "_lib" / "librecsys_hip.so"
HEADER = _PKG.parent / "include" / "recsys_hip.h"

# The header is the only specification: the RS_* constants, the two argument structs and every
# entry point's restype / argtypes are read from it (a type the reader does not know raises here).
CONSTANTS, _STRUCTS, SIGNATURES = read_header(HEADER.read_text())
globals().update(CONSTANTS)  # RS_ID_*, RS_OPT_*, RS_ERRBIT_*, RS_DEDUP_TILE, ...
AdamParams = _STRUCTS["rs_adam_params"]
DlrmTailArgs = _STRUCTS["rs_dlrm_tail_args"]

_lib = None


class RecsysError(RuntimeError):
    pass


def header_symbols() -> list[str]:
    """Every rs_* function declared in include/recsys_hip.h."""
    return sorted(n for n in SIGNATURES if n.startswith("rs_"))


def load(path: str | os.PathLike | None = None):
    """Load the library (no GPU needed). Raises if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    # RS_LIB: A/B runs of a variant build (recommender_amd/build.py --variant)
    p = Path(path) if path else Path(os.environ.get("RS_LIB", LIB_PATH))
    if not p.exists():
        raise RecsysError(f"{p} not built: run `python -m recommender_amd.build` "
                          "(or __graft_entry__.build())")
    lib = C.CDLL(str(p))
    for name, (res, args) in SIGNATURES.items():
        f = getattr(lib, name)
        f.restype = res
        f.argtypes = args
    check_build_id(lib, p)
    _lib = lib
    return lib


def check_build_id(lib, path) -> None:
    """Refuse a library built from other sources than the csrc/ + include/ next to it (the .so
    travels prebuilt, untracked: without this a GPU box could test a stale build of a changed
    kernel with no signal). Skipped when the sources are absent (a library shipped alone)."""
    from .build import CSRC, source_hash

    if not CSRC.is_dir() or os.environ.get("RS_SKIP_BUILD_ID") == "1":
        return
    built, want = lib.rs_build_id().decode(), source_hash()
    if built != want:
        raise RecsysError(f"{path} was built from other sources (build id {built}, sources "
                          f"{want}): rebuild with `python -m recommender_amd.build`")


def lib():
    return _lib if _lib is not None else load()


def check(status: int, fn: str):
    if status != 0:
        msg = lib().rs_last_error().decode(errors="replace")
        raise RecsysError(f"{fn} failed with status {status}: {msg}")


class KernelTimer:
    """Records HIP events around the C-ABI calls named in `names` (on the current stream, the
    stream every kernel is launched on) while enabled; bench.py uses it for per-kernel time."""

    def __init__(self, names):
        self.names = set(names)
        self.events: dict[str, list] = {n: [] for n in self.names}
        self.enabled = False

    def totals_ms(self):
        """{name: (total ms, launches)} over the recorded (eagerly launched) calls."""
        torch.cuda.synchronize()
        return {n: (sum(s.elapsed_time(e) for s, e in ev), len(ev)) for n, ev in self.events.items()}


_timer: KernelTimer | None = None


def set_timer(t: KernelTimer | None):
    global _timer
    _timer = t


def call(fn: str, *args):
    """Invoke a kernel entry point; raises on a non-zero status."""
    f = getattr(lib(), fn)
    t = _timer
    # no events while a stream is being captured: a graph replay does not re-record them, so
    # their elapsed_time would be read off events that never completed (hipErrorInvalidHandle)
    if (t is not None and t.enabled and fn in t.names
            and not torch.cuda.is_current_stream_capturing()):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        st = f(*args)
        e.record()
        t.events[fn].append((s, e))
        check(st, fn)
        return
    check(f(*args), fn)


def require_device(t: torch.Tensor, name: str = "tensor"):
    if not t.is_cuda:
        raise RecsysError(f"{name} must be a GPU tensor (librecsys_hip has no CPU path)")


def ptr(t: torch.Tensor | None):
    return None if t is None else C.c_void_p(t.data_ptr())


def stream_ptr(device=None):
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


class Workspace:
    """Grow-only device scratch buffers (uint8) keyed by name. A buffer is reused by every later
    call under its name, so one Workspace serves calls ordered on one stream. `device` is a
    tensor's device: an index-less torch.device("cuda") equals no buffer's, and would allocate
    anew on every call."""

    def __init__(self):
        self.bufs: dict = {}

    def get(self, name, nbytes, device):
        b = self.bufs.get(name)
        if b is None or b.numel() < nbytes or b.device != device:
            b = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)
            self.bufs[name] = b
        return b


_shared_ws = Workspace()


def workspace(name, nbytes, device):
    """The process-wide buffer of (name, device), for call sites without an owner object; the
    name carries its module's prefix, so no two call sites share a buffer."""
    return _shared_ws.get((name, device), nbytes, device)


def scratch(nbytes, device):
    """A fresh buffer of the nbytes a rs_*_workspace_size() query returned (at least one byte):
    safe on whatever stream the call runs on."""
    return torch.empty(max(1, int(nbytes)), dtype=torch.uint8, device=device)


# Stream ordering with device-scope events (rs_event_*): on by default, RS_DEVICE_EVENTS=0 uses
# torch's default events (a system-scope release at every record) everywhere.
DEVICE_EVENTS = os.environ.get("RS_DEVICE_EVENTS", "1") == "1"


class DeviceEvent:
    """A HIP event whose record is a device-scope release (rs_event_create): it orders the
    engine's own streams of one device without the system-scope cache write-back of a default
    event. Never used for host synchronisation, other devices or other processes. Re-recording
    is allowed once the waits on the previous record are enqueued (a wait binds the record that
    precedes it; on an in-order stream a later record only orders more work)."""
    __slots__ = ("h",)

    def __init__(self):
        h = lib().rs_event_create()
        if not h:
            raise RecsysError(f"rs_event_create: {lib().rs_last_error().decode()}")
        self.h = h

    def record(self, stream):
        call("rs_event_record", C.c_void_p(self.h), C.c_void_p(stream.cuda_stream))

    def wait_by(self, stream):
        call("rs_stream_wait_event", C.c_void_p(stream.cuda_stream), C.c_void_p(self.h))

    def __del__(self):
        try:
            lib().rs_event_destroy(C.c_void_p(self.h))
        except Exception:  # interpreter teardown
            pass


def stream_wait_event(stream, ev):
    """`stream` waits for the record of `ev` (a DeviceEvent or a torch.cuda.Event)."""
    if isinstance(ev, DeviceEvent):
        ev.wait_by(stream)
    else:
        stream.wait_event(ev)


def record_event(stream, ev=None):
    """An event recorded on `stream` now: a DeviceEvent (reused when given) unless device events
    are off or a graph is being captured, else a torch event."""
    if not DEVICE_EVENTS or torch.cuda.is_current_stream_capturing():
        e = torch.cuda.Event()
        e.record(stream)
        return e
    e = ev if isinstance(ev, DeviceEvent) else DeviceEvent()
    e.record(stream)
    return e


def stream_wait_stream(waiter, src, ev=None):
    """`waiter` waits for everything queued on `src` so far (torch's wait_stream, device-scope
    unless device events are off or a graph is being captured); ev: a DeviceEvent to reuse."""
    if waiter == src:
        return
    if not DEVICE_EVENTS or torch.cuda.is_current_stream_capturing():
        waiter.wait_stream(src)
        return
    e = ev if ev is not None else DeviceEvent()
    e.record(src)
    e.wait_by(waiter)


def id_dtype_code(t: torch.Tensor) -> int:
    if t.dtype == torch.int64:
        return RS_ID_I64
    if t.dtype == torch.int32:
        return RS_ID_I32
    raise RecsysError(f"ids must be int32 or int64, got {t.dtype}")
