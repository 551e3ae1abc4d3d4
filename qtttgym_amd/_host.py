"""What VecEnv, TreeSearch, PolicyValueNet and the Board façade share on the host side: which device, the raw stream,
the one way into libqttt_hip.so, the one tensor check and the allocate-or-check helpers for `out=` arguments.
(_native.py stays free of torch; this module is where the two meet.)"""
import math

import numpy as np
import torch

from . import _native

_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
if _raw_stream is None:                                   # older torch: the documented, slower way
    def _raw_stream(index):
        return torch.cuda.current_stream(index).cuda_stream
_current_device = getattr(torch._C, "_cuda_getDevice", torch.cuda.current_device)


def _ptr(t):
    return 0 if t is None else t.data_ptr()


def resolve_device(device, who):
    """`device` as an indexed cuda device: the type must be cuda, a HIP device must be visible, a bare "cuda" is pinned
    to the device that is current now."""
    dev = torch.device(device)
    if dev.type != "cuda":
        raise _native.QtttNativeError("%s runs on an MI355X through libqttt_hip.so only (device=%r); there is no CPU path"
                                      % (who, device))
    if not torch.cuda.is_available():
        raise _native.QtttNativeError("no HIP device visible (torch.cuda.is_available() is False)")
    return dev if dev.index is not None else torch.device("cuda", torch.cuda.current_device())


def check_net(net, dev):
    if getattr(net, "device", None) != dev or not hasattr(net, "blob"):
        raise ValueError("net must be a PolicyValueNet on %s" % (dev,))


class LibCaller:
    """Base of the objects that launch work: `_open(device)` once, then `_call(entry, *args)`."""

    def _open(self, device):
        self.device, self._dev_index, self._lib = device, device.index, _native.lib()

    def _call(self, name, *args):
        """Calls the library's entry `name` with this object's device current and the caller's current stream on it (a
        raw hipStream_t: torch.cuda.current_stream(dev).cuda_stream costs ~3 us per call, the raw lookup ~0.1) as the
        last argument; a non-zero return code raises under the entry's name."""
        fn = getattr(self._lib, name)
        if _current_device() == self._dev_index:
            rc = fn(*args, _raw_stream(self._dev_index))
        else:
            with torch.cuda.device(self.device):
                rc = fn(*args, _raw_stream(self._dev_index))
        if rc:
            _native.check(rc, name)


def check_tensor(t, dtype, shape, dev, what, numel=False):
    """THE test of a tensor whose address goes to a kernel: dtype, device, contiguity and the shape — or, numel=True,
    only the number of elements (any contiguous view of them)."""
    if t.dtype != dtype or t.device != dev or not t.is_contiguous() \
            or (t.numel() != math.prod(shape) if numel else tuple(t.shape) != tuple(shape)):
        raise ValueError("%s must be a contiguous %s tensor of %s %s on %s"
                         % (what, dtype, "the size of shape" if numel else "shape", tuple(shape), dev))
    return t


def out_tensor(dtype, shape, n, dev, out=None, what="out", numel=False):
    """One output of `n` rows of per-board `shape`: allocated, or the caller's `out` checked."""
    if out is None:
        return torch.empty((n,) + shape, dtype=dtype, device=dev)
    return check_tensor(out, dtype, (n,) + shape, dev, what, numel)


def out_tensors(specs, n, dev, out=None, numel=False):
    """The same for a tuple of outputs; specs = ((dtype, per-board shape), ...)."""
    if out is None:
        out = (None,) * len(specs)
    elif len(out) != len(specs):
        raise ValueError("out must hold %d tensors" % len(specs))
    return tuple(out_tensor(dt, shp, n, dev, t, "out[%d]" % i, numel) for i, ((dt, shp), t) in enumerate(zip(specs, out)))


def out_rows(spec, n, dev, out=None, keys=None, required=(), strict=False, numel=False):
    """Named output rows, spec = {name: (dtype, per-board shape)}.  out=None: a new dict with the rows `keys` (default:
    all of spec).  Otherwise the caller's dict is checked and returned: the `required` rows must be there, every row of
    spec it holds must be the right tensor (an entry that is None counts as absent), and — strict — it may hold nothing
    else."""
    if out is None:
        return {k: out_tensor(*spec[k], n, dev) for k in (spec if keys is None else keys)}
    for k in required:
        if out.get(k) is None:
            raise ValueError("out[%r] is required" % k)
    for k, t in out.items():
        if k in spec:
            if t is not None:
                out_tensor(*spec[k], n, dev, t, "out[%r]" % k, numel)
        elif strict:
            raise ValueError("out[%r] is not a row of this call (%s)" % (k, ", ".join(spec)))
    return out


# ---------------------------------------------------------------- the counter hash on the host (include/qttt.h qttt_hash)
_M64 = (1 << 64) - 1


def _splitmix64(x):
    x = (x + 0x9E3779B97F4A7C15) & _M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & _M64
    return x ^ (x >> 31)


def _lowbias32(x):
    with np.errstate(over="ignore"):
        x = (x ^ (x >> np.uint32(16))) * np.uint32(0x7FEB352D)
        x = (x ^ (x >> np.uint32(15))) * np.uint32(0x846CA68B)
        return x ^ (x >> np.uint32(16))


def counter_hash(seed, board_id0, n, idx):
    """qttt_hash(seed, board_id0 + i, idx) for i = 0..n-1 as u64[n] (numpy): the library's counter hash restated for whole
    batches, for the draws that the host makes itself (SelfPlay's playout cap) so that it knows them without a read-back."""
    key = _splitmix64((int(seed) & _M64) ^ (((int(idx) & 0xFFFFFFFF) * 0xD1B54A32D192ED03) & _M64))
    ids = np.arange(n, dtype=np.uint64) + np.uint64(int(board_id0))
    with np.errstate(over="ignore"):
        fold = ids.astype(np.uint32) ^ ((ids >> np.uint64(32)).astype(np.uint32) * np.uint32(0x9E3779B9))    # hi = 0: lo
    h1 = _lowbias32(fold ^ np.uint32(key & 0xFFFFFFFF))
    h2 = _lowbias32(h1 ^ np.uint32(key >> 32))
    return (h2.astype(np.uint64) << np.uint64(32)) | h1.astype(np.uint64)


def cap_full_mask(seed, board_offset, n, ply_index, p):
    """include/qttt_selfplay_cap.h's draw: u8[n] (numpy), 1 where ply number `ply_index` of game g is searched in full:
    (double)(qttt_hash(seed, board_offset + g, QTTT_SELFPLAY_CAP_BASE + ply_index) >> 11) * 2^-53 < p."""
    h = counter_hash(seed, board_offset, n, _native.SELFPLAY_CAP_BASE + int(ply_index))
    return ((h >> np.uint64(11)).astype(np.float64) * 2.0 ** -53 < float(p)).astype(np.uint8)
