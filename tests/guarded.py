"""A guarded arena for the caller-owned buffers of the C ABI (include/kurbm.h), and a DeviceRBM that lives in it.

The header promises that the library writes nothing outside the buffers it is handed, leaves the padding columns [cols, ld) of
its outputs alone, and lets no value of an input's padding reach a result.  The arena makes all three observable:

  * ONE uint8 allocation, filled with 0xFF (a NaN as fp32, bf16 and fp8; non-zero as a byte plane);
  * carve(nbytes): exactly nbytes, 256-byte aligned, a guard of GUARD bytes of 0xFF before and after it;
  * carve_matrix(rows, cols): a DeviceMatrix [rows, ld] with ld % 8 == 4 and ld >= cols + 4 (rows 16-byte but not 32-byte
    aligned, at least one whole 16-byte group of padding).  Inputs: payload copied in, padding left 0xFF.  Outputs: every word
    0xA5A5A5A5 (a finite fp32 no kernel produces), so "left untouched" is checkable;
  * check(): every guard still 0xFF, every output's padding still 0xA5A5A5A5, every frozen buffer byte-identical to the host
    copy taken when it was frozen.  A failure names the buffer, the side and the first and last changed offset.

Nothing here needs a GPU: the arena takes a torch device, and the CPU tier of tests/test_gpu_guard_bands.py shows that check()
fails when a byte is flipped in each of the places it watches.
"""
import numpy as np
import torch

from keras_unsupervised_amd._lib import Params
from keras_unsupervised_amd.ebm.engine import DeviceMatrix, DeviceRBM, round_up

GUARD = 1 << 20
ALIGN = 256
FILL = 0xFF
OUT_WORD = 0xA5A5A5A5
_OUT_I32 = OUT_WORD - (1 << 32)


def wide_ld(cols):
    """Smallest ld with ld % 8 == 4 and ld >= cols + 4."""
    ld = round_up(cols + 4, 4)
    return ld if ld % 8 == 4 else ld + 4


class GuardError(AssertionError):
    pass


class _Buf:
    __slots__ = ("name", "off", "nbytes", "t", "kind", "rows", "cols", "ld", "frozen", "frozen_pad")

    def __init__(self, name, off, nbytes, t):
        self.name, self.off, self.nbytes, self.t = name, off, nbytes, t
        self.kind = "raw"          # raw | input | output | inout
        self.rows = self.cols = self.ld = 0
        self.frozen = None         # host copy of all bytes (must stay identical)
        self.frozen_pad = None     # host copy of the padding columns alone (inout matrices)


class Arena:
    def __init__(self, device, capacity=192 << 20, guard=GUARD):
        self.device = torch.device(device)
        self.guard = int(guard)
        self.buf = torch.full((int(capacity) + ALIGN,), FILL, dtype=torch.uint8, device=self.device)
        self.base = (-self.buf.data_ptr()) % ALIGN       # offset of the first 256-byte aligned byte
        self.cursor = self.base
        self.bufs = []
        self._names = set()

    # -- carving ------------------------------------------------------------------------------------------------------
    def _name(self, name):
        name, n = name or "buf", 1
        base = name
        while name in self._names:
            n += 1
            name = "%s#%d" % (base, n)
        self._names.add(name)
        return name

    def carve(self, nbytes, name=None):
        """A uint8 tensor of exactly nbytes (all 0xFF), 256-byte aligned, GUARD bytes of 0xFF on either side."""
        nbytes = int(nbytes)
        assert nbytes > 0
        off = round_up(self.cursor + self.guard - self.base, ALIGN) + self.base
        end = off + nbytes
        if end + self.guard > self.buf.numel():
            raise MemoryError("arena of %d bytes is full (carving %d for %r)" % (self.buf.numel(), nbytes, name))
        self.cursor = end + self.guard      # the guards of two neighbours do not overlap: a changed byte has one owner
        t = self.buf[off:end]
        assert t.data_ptr() % ALIGN == 0 and t.numel() == nbytes
        b = _Buf(self._name(name), off, nbytes, t)
        self.bufs.append(b)
        return t

    def _rec(self, t):
        ptr = t.t.data_ptr() if isinstance(t, DeviceMatrix) else t.data_ptr()
        for b in self.bufs:
            if b.t.data_ptr() == ptr:
                return b
        raise KeyError("not a carve of this arena")

    def carve_floats(self, n, name=None, data=None, zero=False, dtype=torch.float32):
        """A dense vector of n 4-byte words: NaN (0xFF) unless `zero` or `data` (a host array copied in)."""
        t = self.carve(4 * int(n), name).view(dtype)
        if data is not None:
            t.copy_(torch.from_numpy(np.ascontiguousarray(data).reshape(-1)).to(dtype))
        elif zero:
            t.zero_()
        return t

    def carve_matrix(self, rows, cols, wide=True, data=None, name=None, kind=None):
        """A DeviceMatrix over an fp32 [rows, ld] carve.  data given: an input (kind 'input', or 'inout' for a matrix the
        library also writes, such as W or a persistent chain) -- payload copied in, padding 0xFF.  No data: an output, every
        word 0xA5A5A5A5."""
        rows, cols = int(rows), int(cols)
        ld = wide_ld(cols) if wide else round_up(cols, 4)
        t = self.carve(4 * rows * ld, name).view(torch.float32).view(rows, ld)
        b = self.bufs[-1]
        b.rows, b.cols, b.ld = rows, cols, ld
        if data is None:
            b.kind = kind or "output"
            t.view(torch.int32).fill_(_OUT_I32)
        else:
            b.kind = kind or "input"
            src = torch.from_numpy(np.ascontiguousarray(np.asarray(data), dtype=np.float32))
            assert tuple(src.shape) == (rows, cols), (tuple(src.shape), rows, cols)
            t[:, :cols].copy_(src)
        m = DeviceMatrix(t, rows, cols, ld)
        if b.kind == "input":
            self.freeze(m)
        elif b.kind == "inout":
            b.frozen_pad = t[:, cols:].contiguous().view(torch.uint8).cpu().clone()
        return m

    def freeze(self, t):
        """From now on check() wants every byte of this carve identical to what it holds at this moment."""
        b = self._rec(t)
        b.frozen = b.t.cpu().clone()
        return t

    def thaw(self, t):
        self._rec(t).frozen = None

    def freeze_all(self):
        """Freeze every carve (a refused call must change nothing at all)."""
        for b in self.bufs:
            b.frozen = b.t.cpu().clone()

    # -- checking -----------------------------------------------------------------------------------------------------
    @staticmethod
    def _span(bad):
        idx = bad.reshape(-1).nonzero().reshape(-1)
        return int(idx[0].item()), int(idx[-1].item()), int(idx.numel())

    def problems(self):
        out = []
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        # one pass over the whole arena first: the usual answer is "every guard byte is still 0xFF"
        mask = torch.ones(self.buf.numel(), dtype=torch.bool, device=self.device)
        for b in self.bufs:
            mask[b.off:b.off + b.nbytes] = False
        if bool(((self.buf != FILL) & mask).any().item()):
            for b in self.bufs:
                lo, hi = b.off - self.guard, b.off + b.nbytes + self.guard
                if b is self.bufs[0]:
                    lo = 0
                if b is self.bufs[-1]:
                    hi = self.buf.numel()
                for side, a, z in (("leading guard", lo, b.off), ("trailing guard", b.off + b.nbytes, hi)):
                    bad = self.buf[a:z] != FILL
                    if bool(bad.any().item()):
                        first, last, n = self._span(bad)
                        out.append("%s: %s changed, %d bytes, offsets %d .. %d relative to the buffer (of %d bytes)"
                                   % (b.name, side, n, a + first - b.off, a + last - b.off, b.nbytes))
            if not self.bufs:
                out.append("arena: bytes changed although nothing is carved")
        for b in self.bufs:
            if b.kind == "output" and b.ld > b.cols:
                m = b.t.view(torch.int32).view(b.rows, b.ld)
                bad = m[:, b.cols:] != _OUT_I32
                if bool(bad.any().item()):
                    rc = bad.nonzero()
                    offs = (rc[:, 0] * b.ld + b.cols + rc[:, 1]) * 4
                    out.append("%s: output padding changed, %d words, byte offsets %d .. %d relative to the buffer (first at row %d, "
                               "column %d of ld %d, %d columns)" % (b.name, int(rc.shape[0]), int(offs.min().item()), int(offs.max().item()) + 3,
                                                                   int(rc[0, 0].item()), b.cols + int(rc[0, 1].item()), b.ld, b.cols))
            if b.frozen_pad is not None and b.frozen is None:
                now = b.t.view(torch.float32).view(b.rows, b.ld)[:, b.cols:].contiguous().view(torch.uint8).cpu()
                bad = now != b.frozen_pad
                if bool(bad.any().item()):
                    rc = bad.reshape(b.rows, -1).nonzero()
                    offs = rc[:, 0] * b.ld * 4 + b.cols * 4 + rc[:, 1]
                    out.append("%s: input padding changed, %d bytes, offsets %d .. %d relative to the buffer"
                               % (b.name, int(rc.shape[0]), int(offs.min().item()), int(offs.max().item())))
            if b.frozen is not None:
                bad = b.t.cpu() != b.frozen
                if bool(bad.any().item()):
                    first, last, n = self._span(bad)
                    where = ""
                    if b.ld:
                        col = (first // 4) % b.ld
                        where = " (first in the %s, row %d, column %d)" % ("padding" if col >= b.cols else "payload", first // 4 // b.ld, col)
                    out.append("%s: input contents changed, %d bytes, offsets %d .. %d relative to the buffer%s" % (b.name, n, first, last, where))
        return out

    def check(self):
        bad = self.problems()
        if bad:
            raise GuardError("arena check failed:\n  " + "\n  ".join(bad))


class GuardedRBM(DeviceRBM):
    """A DeviceRBM every buffer of which is an arena carve of exactly the queried size: W with a wide ldw and NaN padding,
    b_h, b_v, workspaces, mirrors, delta, velocity, resident planes, F / score words and output matrices (wide ld_out).
    Scratch the library is to write before it reads (workspaces, mirrors, planes, delta) starts as 0xFF, not zero."""

    def __init__(self, arena, W, b_h, b_v, device=None):
        self.arena = arena
        super().__init__(W, b_h, b_v, device)
        with torch.cuda.device(self.device):
            self.W = arena.carve_matrix(self.n_vis, self.n_hid, data=W, name="W", kind="inout")
            self.b_h = arena.carve_floats(self.n_hid, "b_h", data=np.asarray(b_h, dtype=np.float32))
            self.b_v = arena.carve_floats(self.n_vis, "b_v", data=np.asarray(b_v, dtype=np.float32))
        self.params = Params(self.n_vis, self.n_hid, self.W.ld, 0, self.W.t.data_ptr(), self.b_h.data_ptr(), self.b_v.data_ptr())

    def _alloc_bytes(self, n, what, zero=True):
        return self.arena.carve(n, what)

    def _alloc_floats(self, n, what, zero=True):
        return self.arena.carve_floats(n, what, zero=(zero and what == "velocity"))

    def _alloc_out(self, rows, cols, what):
        return self.arena.carve_matrix(rows, cols, name="out_" + what)

    def freeze_params(self, W=True, b_h=True, b_v=True):
        """The call that follows must not write these parameters at all (a half step; a `which` that leaves them out)."""
        for t, on in ((self.W, W), (self.b_h, b_h), (self.b_v, b_v)):
            if on:
                self.arena.freeze(t)
