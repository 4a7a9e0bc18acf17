"""Guarded arenas: every buffer of a call carved out of one allocation, so that a store outside
the bytes a call owns is read back instead of landing in allocator slack.

include/shipenv.h states every buffer's size ("n entries each", "m entries", "2 * segments
counts") and what a call leaves alone ("only read", "not modified", "not written"). An Arena lays
the buffers of one call out as

    guard | buffer | guard   guard | buffer | guard   ...

with every buffer starting 16-byte aligned (or, with odd=True for the host stepper, one byte past
that), exactly as many bytes long as the header documents, its trailing guard beginning at the
very next byte, and every guard at least GUARD = 4 KiB: twice the widest row one wave stores with
one instruction (64 lanes x 32 B, the fuel store of st4_full in csrc/step_io.h), so a whole
misplaced wave still lands inside a guard and inside the allocation. Guards hold a
position-dependent, never-zero byte pattern; outputs a second one (fill_out), so "not written" is
checkable per entry; inputs and read-only state are compared with a snapshot, as bytes.

numpy alone on the CPU (test_footprint_support_cpu.py); with device= the allocation is one torch
uint8 tensor and view() hands out typed tensor views into it (test_gpu_footprint.py). All checks
run on one host copy of the arena.
"""
import ctypes as C

import numpy as np

GUARD = 4096
ALIGN = 16

STATE_FIELDS = (  # se_state, in the order of include/shipenv.h; the u8 fields first in the arena
    ("x", np.uint8), ("y", np.uint8), ("origin", np.uint8), ("dest", np.uint8), ("done", np.uint8),
    ("err", np.int8), ("fuel", np.float64), ("cargo", np.int32), ("reward", np.float32),
    ("ep_return", np.float32), ("ep_start", np.int32))
BIND_ORDER = ("x", "y", "fuel", "cargo", "origin", "dest", "reward", "done", "err", "ep_return", "ep_start",
              "done_recs", "done_count")


def guard_pattern(pos):
    """The guard byte at arena position pos: 1..251, never zero, never constant."""
    return ((np.asarray(pos, np.int64) * 37 + 11) % 251 + 1).astype(np.uint8)


def out_pattern(pos):
    """The output prefill at arena position pos: 57..255, another sequence than the guards'."""
    return (255 - (np.asarray(pos, np.int64) * 13 + 5) % 199).astype(np.uint8)


class Buf:
    def __init__(self, name, dtype, shape, start, nbytes, lo, hi):
        self.name, self.dtype, self.shape = name, np.dtype(dtype), shape
        self.start, self.nbytes = start, nbytes  # the buffer is arena[start : start + nbytes]
        self.lo, self.hi = lo, hi                # its guards are arena[lo : start] and arena[end : hi]

    @property
    def end(self):
        return self.start + self.nbytes


class Arena:
    """Arena([(name, dtype, shape), ...], device=None, odd=False). shape: an int or a tuple; a
    zero-sized buffer is legal (its two guards then touch)."""

    def __init__(self, specs, device=None, odd=False):
        self.bufs, self.device = {}, device
        cur = 0
        for name, dtype, shape in specs:
            shape = (int(shape),) if np.isscalar(shape) else tuple(int(s) for s in shape)
            nbytes = int(np.prod(shape, dtype=np.int64)) * np.dtype(dtype).itemsize
            start = -(-(cur + GUARD) // ALIGN) * ALIGN + (1 if odd else 0)
            assert name not in self.bufs, name
            self.bufs[name] = Buf(name, dtype, shape, start, nbytes, cur, start + nbytes + GUARD)
            cur = start + nbytes + GUARD
        self.size = cur
        if device is None:
            raw = np.zeros(self.size + ALIGN, np.uint8)
            skew = (-raw.ctypes.data) % ALIGN
            self.mem = raw[skew:skew + self.size]
            self.base = self.mem.ctypes.data
        else:
            import torch

            self.mem = torch.zeros(self.size, dtype=torch.uint8, device=device)
            self.base = self.mem.data_ptr()
        assert self.base % ALIGN == 0
        pos = np.arange(self.size)
        image = guard_pattern(pos)
        for b in self.bufs.values():
            image[b.start:b.end] = out_pattern(pos[b.start:b.end])
        self._put(0, image)
        self._image0 = image  # guards and prefill as laid down: what untouched bytes still hold
        self._guard = np.ones(self.size, bool)
        for b in self.bufs.values():
            self._guard[b.start:b.end] = False
        self._snap = None

    # ------------------------------------------------------------------ access
    def _put(self, at, data):
        data = np.ascontiguousarray(data).view(np.uint8).reshape(-1)
        if self.device is None:
            self.mem[at:at + len(data)] = data
        else:
            import torch

            self.mem[at:at + len(data)].copy_(torch.from_numpy(data.copy()))

    def host(self):
        """The whole arena as host bytes (a copy; on a device, after a synchronise)."""
        if self.device is None:
            return self.mem.copy()
        import torch

        torch.cuda.synchronize(self.device)
        return self.mem.cpu().numpy()

    def ptr(self, name):
        return self.base + self.bufs[name].start

    def cptr(self, name):
        return C.c_void_p(self.ptr(name))

    def view(self, name):
        """The buffer as a typed view into the arena (numpy array or torch tensor): writes through it
        land in the arena, and the bytes past its last entry are the trailing guard."""
        b = self.bufs[name]
        raw = self.mem[b.start:b.end]
        if self.device is None:
            # an odd start is unaligned for the dtype: numpy views it all the same
            return np.ndarray(b.shape, b.dtype, buffer=self.mem.data, offset=b.start) if b.nbytes else \
                np.zeros(b.shape, b.dtype)
        import torch

        tdt = getattr(torch, b.dtype.name)
        return raw.view(tdt).reshape(b.shape)

    def set(self, name, values):
        """Write an input: values cast to the buffer's dtype, exactly its shape."""
        b = self.bufs[name]
        v = np.ascontiguousarray(np.broadcast_to(np.asarray(values).astype(b.dtype), b.shape))
        self._put(b.start, v)

    def get(self, name, image=None):
        """The buffer's current content as a numpy array (from `image`, a host() copy, if given)."""
        b = self.bufs[name]
        image = self.host() if image is None else image
        return image[b.start:b.end].copy().view(b.dtype).reshape(b.shape)

    def fill_out(self, *names):
        for name in names or self.bufs:
            b = self.bufs[name]
            self._put(b.start, self._image0[b.start:b.end])

    def prefill(self, name):
        """What fill_out leaves in the buffer, as its dtype."""
        b = self.bufs[name]
        return self._image0[b.start:b.end].copy().view(b.dtype).reshape(b.shape)

    def unwritten(self, name, image=None):
        """Per entry (first axis folded to the buffer's shape): does it still hold the prefill?"""
        b = self.bufs[name]
        image = self.host() if image is None else image
        same = image[b.start:b.end] == self._image0[b.start:b.end]
        return same.reshape(b.shape + (b.dtype.itemsize,)).all(-1)

    # ------------------------------------------------------------------ checks
    def snapshot(self):
        """Remember every byte: check(unchanged=...) compares buffers against this."""
        self._snap = self.host()
        return self._snap

    def check(self, unchanged=(), image=None):
        """-> a list of findings, empty when every guard holds its pattern and every buffer named in
        `unchanged` equals the snapshot byte for byte. A damaged guard is named by buffer, side and
        the first and last changed offset, counted from the buffer's first byte (before: negative)
        or from its end (after: from 0)."""
        image = self.host() if image is None else image
        found = []
        damaged = ((image != self._image0) & self._guard).any()
        for b in self.bufs.values() if damaged else ():
            for side, lo, hi, origin in (("before", b.lo, b.start, b.start), ("after", b.end, b.hi, b.end)):
                bad = np.nonzero(image[lo:hi] != self._image0[lo:hi])[0]
                if len(bad):
                    found.append(f"{b.name}: guard {side} the buffer damaged, offsets {lo + bad[0] - origin}"
                                 f"..{lo + bad[-1] - origin} ({len(bad)} bytes)")
        for name in unchanged:
            assert self._snap is not None, "check(unchanged=...) needs a snapshot()"
            b = self.bufs[name]
            bad = np.nonzero(image[b.start:b.end] != self._snap[b.start:b.end])[0]
            if len(bad):
                size = b.dtype.itemsize
                found.append(f"{b.name}: content changed, bytes {bad[0]}..{bad[-1]} (entries {bad[0] // size}"
                             f"..{bad[-1] // size}, {len(bad)} bytes)")
        return found

    def assert_clean(self, unchanged=(), image=None, what=""):
        found = self.check(unchanged, image)
        assert not found, f"{what}: " + "; ".join(found)


# ---------------------------------------------------------------------- the guarded env
def state_specs(n, nrec, ncount):
    """The thirteen se_state buffers at their documented sizes: n entries each, nrec done records
    of 16 bytes, ncount counts."""
    return [(f, dt, n) for f, dt in STATE_FIELDS] + [("done_recs", np.int32, (nrec, 4)), ("done_count", np.int32, ncount)]


def guard_env(env, extra=()):
    """Rebind a fresh VecEnv to views into one device arena: its state tensors at exactly n
    entries, done_recs at exactly 2 * segments * seg_stride records and done_count at 2 * segments
    counts (se_done_layout), then the call's own buffers `extra`. Every state buffer comes out
    holding the output prefill. se_bind after se_create is legal; with auto-reset it clears the
    counts, so the caller prefills done_recs / done_count after this (and after set_counters)."""
    from shippingenv_amd import _native as N

    nrec = 2 * env.done_segments * env.done_seg
    arena = Arena(state_specs(env.n, nrec, 2 * env.done_segments) + list(extra), device=env.device)
    for f in BIND_ORDER:
        setattr(env, f, arena.view(f))
    env._state = N.SeState(*[arena.ptr(f) for f in BIND_ORDER] + [None])
    N.check(N.lib().se_bind(env._h, C.byref(env._state)))
    return arena
