"""Device-side state of one RBM and the ctypes calls that drive the HIP kernels.

PyTorch is used for exactly three things here: owning device memory (``torch.zeros`` /
``data_ptr()``), naming the current HIP stream, and host<->device copies.  All arithmetic
of the contrastive-divergence path happens inside ``libkurbm.so``.
"""
import ctypes as C

import numpy as np
import torch

from .. import _lib
from .._lib import (ACT_LINEAR, ACT_RELU, ACT_SIGMOID, NOISE_BERNOULLI, NOISE_GAUSSIAN, NOISE_NONE,
                    WHICH_ALL, CdOpts, Context, Momentum, Params, Rng, check)

MODE_VISIBLE_BERNOULLI = 0
MODE_VISIBLE_GAUSSIAN = 1
MODE_COMPLEX = 2

# sampling-site ids of the RNG contract (include/kurbm.h; CPU statement: oracle/rbm_oracle.py)
CHAIN_STRIDE = 64
STREAM_TRANSFORM = 0x100
STREAM_INV_TRANSFORM = 0x101
# the three sites of an AIS run (kurbm_ais_run): v_0 (step 0), then h and v of temperature k (step k); row = the chain's index
STREAM_AIS_INIT = 0x200
STREAM_AIS_H = 0x201
STREAM_AIS_V = 0x202
# the two sites of a Gibbs run (kurbm_gibbs_run): h and v of sweep t (step t); row = the chain's index
STREAM_GIBBS_H = 0x210
STREAM_GIBBS_V = 0x211
CHAIN_W, CHAIN_BH, CHAIN_BV, CHAIN_SCORE = 0, 1, 2, 3


def round_up(x, m):
    return (x + m - 1) // m * m


def clamp_mask(clamp, n_vis):
    """A clamp argument as a host uint8 mask [n_vis] (1 = clamped): a BOOLEAN mask of that length, or a list of unit indices
    (integers; an integer array is always read as indices)."""
    a = clamp.detach().cpu().numpy() if isinstance(clamp, torch.Tensor) else np.asarray(clamp)
    if a.dtype == np.bool_:
        if a.shape != (n_vis,):
            raise ValueError("clamp mask has shape %s, the RBM has %d visible units" % (a.shape, n_vis))
        return np.ascontiguousarray(a != 0, dtype=np.uint8)
    idx = a.reshape(-1)
    if idx.size and idx.dtype.kind not in "iu":
        raise ValueError("clamp must be a boolean mask [n_vis] or a list of unit indices")
    idx = idx.astype(np.int64)
    if idx.size and (idx.min() < 0 or idx.max() >= n_vis):
        raise ValueError("clamp index out of range for %d visible units" % n_vis)
    m = np.zeros(n_vis, np.uint8)
    m[idx] = 1
    return m


def resolve_device(device=None):
    """The gfx950 device this process drives.  No GPU -> loud failure (no CPU path exists)."""
    if not torch.cuda.is_available():
        raise _lib.KurbmError(
            "no ROCm device visible: keras_unsupervised_amd runs its RBM/DBN path on MI355X (gfx950) "
            "HIP kernels only and has no CPU fallback")
    if device is None:
        return torch.device("cuda", torch.cuda.current_device())
    device = torch.device(device)
    if device.type != "cuda":
        raise _lib.KurbmError("device must be a ROCm ('cuda') device, got %s" % device)
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    return device


def device_guard(device):
    """`with` context that makes a ROCm device current (a no-op for any other device type)."""
    import contextlib
    return torch.cuda.device(device) if torch.device(device).type == "cuda" else contextlib.nullcontext()


class DeviceMatrix:
    """Row-major fp32 [rows, ld] matrix on the device, ld % 4 == 0, padding zero."""

    __slots__ = ("t", "rows", "cols", "ld", "bf16_exact", "binary")

    def __init__(self, t, rows, cols, ld):
        self.t, self.rows, self.cols, self.ld = t, rows, cols, ld
        self.bf16_exact = None   # True / False once DeviceRBM.v_pieces() has looked (0/1 data is exact)
        self.binary = None       # ... and whether every element is 0.0 or 1.0

    @classmethod
    def zeros(cls, rows, cols, device):
        ld = round_up(cols, 4)
        return cls(torch.zeros((max(rows, 1), ld), dtype=torch.float32, device=device), rows, cols, ld)

    @classmethod
    def from_host(cls, x, device):
        """Upload a numpy / torch [rows, cols] array (any float dtype) as fp32."""
        if isinstance(x, torch.Tensor):
            src = x.detach().to(dtype=torch.float32)
        else:
            src = torch.from_numpy(np.ascontiguousarray(np.asarray(x), dtype=np.float32))
        if src.dim() != 2:
            raise ValueError("expected a 2-d array, got shape %s" % (tuple(src.shape),))
        rows, cols = src.shape
        ld = round_up(cols, 4)
        if isinstance(x, torch.Tensor) and src.is_cuda and ld == cols and src.is_contiguous() \
                and src.data_ptr() % 16 == 0 and src.device == device:
            return cls(src, rows, cols, ld)  # already in the device layout: no copy
        m = cls.zeros(rows, cols, device)
        m.t[:rows, :cols].copy_(src, non_blocking=False)
        return m

    def ptr(self, row=0):
        return self.t.data_ptr() + row * self.ld * 4

    def to_numpy(self):
        return self.t[: self.rows, : self.cols].contiguous().cpu().numpy()      # (rows may be 0: an empty [0, cols] array)

    def view(self):
        """[rows, cols] torch view (device)."""
        return self.t[: self.rows, : self.cols]


class ResidentPlanes:
    """bf16 planes (kurbm_x3_convert_rows) of windows of rows of a data matrix, made once and read by every x3 step on
    those rows instead of a per-step conversion: fit() walks the same windows every epoch (rbm.py:113, :211)."""

    def __init__(self, eng, v, windows, v_pieces):
        self.v, self.v_pieces = v, int(v_pieces)
        self.windows = [(int(lo), int(rows)) for lo, rows in windows]
        max_rows = max([rows for _, rows in self.windows] + [1])
        self.stride = int(eng.lib.kurbm_x3_planes_bytes(eng.ctx.handle, max_rows, eng.n_vis, self.v_pieces))
        if self.stride == 0:
            raise _lib.KurbmError("kurbm_x3_planes_bytes failed")
        self.buf = eng._alloc_bytes(max(len(self.windows), 1) * self.stride, "planes", zero=False)
        self.slot = {}
        for t, (lo, rows) in enumerate(self.windows):
            if rows <= 0:
                continue
            check(eng.lib.kurbm_x3_convert_rows(eng.ctx.handle, v.ptr(lo), rows, v.ld, eng.n_vis, self.v_pieces,
                                                self.buf.data_ptr() + t * self.stride, self.stride, eng._stream()))
            self.slot[(lo, rows)] = t

    def ptr(self, v, row_start, rows, v_pieces):
        """Device address of the planes of rows [row_start, +rows) of v, or None if these are not planes of them."""
        t = self.slot.get((int(row_start), int(rows)))
        if t is None or v is not self.v or v_pieces != self.v_pieces:
            return None
        return self.buf.data_ptr() + t * self.stride

    def uniform(self, row_start, n_rows, batch_size):
        """True if the windows are exactly the contiguous batches of rows [row_start, +n_rows) (kurbm_cd_epoch_x3)."""
        want = [(row_start + lo, min(batch_size, n_rows - lo)) for lo in range(0, n_rows, batch_size)]
        return want == self.windows


class DeviceRBM:
    """W, b_h, b_v on one device + scratch, and one method per C-ABI entry point."""

    def __init__(self, W, b_h, b_v, device=None):
        self.device = resolve_device(device)
        self.ctx = Context.get(self.device.index)
        self.lib = self.ctx.lib
        W = np.asarray(W, dtype=np.float32)
        self.n_vis, self.n_hid = W.shape
        with torch.cuda.device(self.device):
            self.W = DeviceMatrix.from_host(W, self.device)
            if self.W.t.data_ptr() == 0:
                raise _lib.KurbmError("device allocation failed")
            self.b_h = torch.from_numpy(np.ascontiguousarray(b_h, dtype=np.float32)).to(self.device)
            self.b_v = torch.from_numpy(np.ascontiguousarray(b_v, dtype=np.float32)).to(self.device)
        assert self.b_h.numel() == self.n_hid and self.b_v.numel() == self.n_vis
        self.params = Params(self.n_vis, self.n_hid, self.W.ld, 0, self.W.t.data_ptr(),
                             self.b_h.data_ptr(), self.b_v.data_ptr())
        self._ws = None
        self._ws_rows = 0
        self._ws_ldv = 0
        self.delta = None  # packed [V*H | H | V] sums, allocated on first use
        # bf16 images of W in both orientations, per number of pieces: 1 = rounded (compute 'bf16'),
        # 3 = exact hi/mid/lo split (compute 'x3');  [tensor, stale]
        self._mirrors = {}
        self._ws_b = {}
        self._ws_disc = None   # (key, rows, buffer): the scratch of disc_step / disc_epoch
        self._ws_bp = None     # (rows, buffer): the scratch of backprop_layer
        self.velocity = None   # packed [V*H | H | V] fp32 velocity of the momentum steps, allocated (zero) on first use

    # -- plumbing -------------------------------------------------------------------
    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    # Every buffer the library is handed besides the parameters comes from one of these three (`what` names its use).  A subclass
    # may place them elsewhere (tests/guarded.py carves them out of a guarded arena, each exactly as large as its size query says).
    def _alloc_bytes(self, n, what, zero=True):
        """Raw device bytes: workspaces, mirrors, resident planes."""
        return (torch.zeros if zero else torch.empty)(n, dtype=torch.uint8, device=self.device)

    def _alloc_floats(self, n, what, zero=True):
        """A dense fp32 device vector: packed delta / velocity, free energies, the score words, a dense dW."""
        return (torch.zeros if zero else torch.empty)(n, dtype=torch.float32, device=self.device)

    def _alloc_out(self, rows, cols, what):
        """An output DeviceMatrix [rows, cols]; its ld is what the library is given."""
        return DeviceMatrix.zeros(rows, cols, self.device)

    def workspace(self, rows, k=1, ldv=0):
        """Scratch of the fp32 entry points for batches of <= rows.  ldv: the leading dimension of the batch of a kurbm_cd_step /
        kurbm_cd_epoch when it exceeds round_up(n_vis, 4) -- the step keeps v_neg at that leading dimension and needs that much more
        (include/kurbm.h, kurbm_workspace_bytes); a DeviceMatrix made here never does."""
        ldc = round_up(self.n_vis, 4)
        ldv = max(int(ldv), ldc, self._ws_ldv)
        if self._ws is None or rows > self._ws_rows or ldv > self._ws_ldv:
            rows = max(rows, self._ws_rows)
            n = self.lib.kurbm_workspace_bytes(self.ctx.handle, rows, self.n_vis, self.n_hid, k)
            if n == 0:
                raise _lib.KurbmError("kurbm_workspace_bytes failed")
            n += round_up(rows * ldv * 4, 256) - round_up(rows * ldc * 4, 256)
            self._ws = self._alloc_bytes(n, "workspace")
            self._ws_rows, self._ws_ldv = rows, ldv
        return self._ws

    def delta_buffer(self):
        if self.delta is None:
            n = self.n_vis * self.n_hid + self.n_hid + self.n_vis
            self.delta = self._alloc_floats(n, "delta")
        return self.delta

    # -- momentum / weight decay (include/kurbm.h: kurbm_momentum) -------------------------------
    def velocity_buffer(self):
        if self.velocity is None:
            n = self.n_vis * self.n_hid + self.n_hid + self.n_vis
            with torch.cuda.device(self.device):
                self.velocity = self._alloc_floats(n, "velocity")
        return self.velocity

    def _mom(self, momentum):
        """The kurbm_momentum block of a `momentum=` keyword: (mu, weight_decay), or mu alone.  The rule, all fp32:
        vel <- mu vel + lr (g - weight_decay W); W <- W + vel (biases: no decay), g = the batch SUMS -- so weight_decay is on
        the scale of those sums (lr multiplies sums: rbm.py:128), not of a per-row mean."""
        mu, decay = momentum if isinstance(momentum, (tuple, list)) else (momentum, 0.0)
        return Momentum(float(mu), float(decay), self.velocity_buffer().data_ptr())

    def get_velocity(self):
        """(vel_W [n_vis, n_hid], vel_b_h, vel_b_v) as host arrays, or None when no momentum step has run (or set_velocity)."""
        if self.velocity is None:
            return None
        v, nw = self.velocity.cpu().numpy(), self.n_vis * self.n_hid
        return v[:nw].reshape(self.n_vis, self.n_hid).copy(), v[nw:nw + self.n_hid].copy(), v[nw + self.n_hid:].copy()

    def set_velocity(self, W=None, b_h=None, b_v=None):
        buf, nw = self.velocity_buffer(), self.n_vis * self.n_hid
        for x, lo, n in ((W, 0, nw), (b_h, nw, self.n_hid), (b_v, nw + self.n_hid, self.n_vis)):
            if x is not None:
                x = np.ascontiguousarray(x, dtype=np.float32).reshape(-1)
                assert x.size == n
                buf[lo:lo + n].copy_(torch.from_numpy(x))

    # -- bf16 mirrors (fp32 master weights stay authoritative) --------------------------------
    def _weights_written(self, kept=None):
        """The fp32 W changed; every mirror except the one the library refreshed itself is stale."""
        for pieces, m in self._mirrors.items():
            if pieces != kept:
                m[1] = True

    def mirror(self, pieces=1):
        """The bf16 images of W (1 piece: rounded; 3: exact split), refreshed if W was written elsewhere."""
        m = self._mirrors.get(pieces)
        fn_bytes = self.lib.kurbm_bf16_mirror_bytes if pieces == 1 else self.lib.kurbm_x3_mirror_bytes
        fn_refresh = self.lib.kurbm_bf16_mirror_refresh if pieces == 1 else self.lib.kurbm_x3_mirror_refresh
        if m is None:
            n = fn_bytes(self.ctx.handle, self.n_vis, self.n_hid)
            m = self._mirrors[pieces] = [self._alloc_bytes(n, "mirror%d" % pieces), True]
        if m[1]:
            check(fn_refresh(self.ctx.handle, C.byref(self.params), m[0].data_ptr(), m[0].numel(), self._stream()))
            m[1] = False
        return m[0]

    def workspace_bf16(self, rows, k=1, pieces=1, v_pieces=1):
        key = (pieces, v_pieces)
        have = self._ws_b.get(key)
        if have is None or rows > have[1]:
            if pieces == 1:
                n = self.lib.kurbm_bf16_workspace_bytes(self.ctx.handle, rows, self.n_vis, self.n_hid, k)
            else:
                n = self.lib.kurbm_x3_workspace_bytes(self.ctx.handle, rows, self.n_vis, self.n_hid, k, v_pieces)
            if n == 0:
                raise _lib.KurbmError("workspace size query failed")
            have = self._ws_b[key] = (self._alloc_bytes(n, "workspace%d" % pieces), rows)
        return have[0]

    def v_pieces(self, v):
        """1 if every element of DeviceMatrix v is exactly a bf16 value (0/1 data is), else 3.

        Looked at once per matrix (one pass over it on the device, one 4-byte read back)."""
        if v.bf16_exact is None:
            with torch.cuda.device(self.device):
                flag = torch.zeros(1, dtype=torch.int32, device=self.device)
                check(self.lib.kurbm_bf16_exact(self.ctx.handle, v.ptr(), max(v.rows, 1), v.cols, v.ld, flag.data_ptr(),
                                                self._stream()))
                bits = int(flag.item())
                v.bf16_exact, v.binary = (bits & 1) == 0, bits == 0
        return 1 if v.bf16_exact else 3

    def check_status(self):
        """Raise if a kernel of this context reported a problem (kurbm_ctx_status; synchronises with the device).  Bits 1 and 2
        mean a device-side wait ran into its bound and an update was SKIPPED -- training must not go on from that state: bit 1 =
        the peer exchange (a rank never arrived), bit 2 = a barrier of the one-launch small step or score (its grid was not
        resident: a CU mask, a device shared with another process -- or the dispatcher did not deal its workgroups to the XCDs
        in turn: KURBM_SMALL_LOCAL=0 takes the grid-wide schedule)."""
        bits = self.ctx.status()
        if bits:
            what = [name for bit, name in ((2, "the peer exchange timed out waiting for a rank"),
                                           (4, "the one-launch small step found its grid not resident")) if bits & bit]
            raise _lib.KurbmError("kurbm status %#x: %s; an update was skipped and the replicas / weights are no longer what the "
                                  "step sequence defines -- reload the weights (set_weights)" % (bits, "; ".join(what) or "unknown bit"))

    def get_weights(self):
        out = self.W.to_numpy(), self.b_h.cpu().numpy(), self.b_v.cpu().numpy()     # (device -> host copies: a sync)
        self.check_status()
        return out

    def set_weights(self, W=None, b_h=None, b_v=None):
        if W is not None:
            W = np.asarray(W, dtype=np.float32)
            assert W.shape == (self.n_vis, self.n_hid)
            self.W.t[:, : self.n_hid].copy_(torch.from_numpy(np.ascontiguousarray(W)))
            self._weights_written()
        if b_h is not None:
            self.b_h.copy_(torch.from_numpy(np.ascontiguousarray(b_h, dtype=np.float32)))
        if b_v is not None:
            self.b_v.copy_(torch.from_numpy(np.ascontiguousarray(b_v, dtype=np.float32)))

    # -- kernels --------------------------------------------------------------------
    def half_step(self, direction, x, rows, row_start, act, noise, seed, stream_id, step, row0=0,
                  want_sample=True, want_prob=False, want_u=False):
        """One fused half step over rows [row_start, row_start+rows) of DeviceMatrix x.

        direction 'vh': x is [*, n_vis] -> outputs [rows, n_hid];  'hv': the converse.
        Returns dict of DeviceMatrix for the requested outputs.
        """
        n_out = self.n_hid if direction == "vh" else self.n_vis
        n_in = self.n_vis if direction == "vh" else self.n_hid
        if x.cols != n_in:
            raise ValueError("input has %d columns, expected %d" % (x.cols, n_in))
        out = {}
        with torch.cuda.device(self.device):
            for key, want in (("sample", want_sample), ("prob", want_prob), ("u", want_u)):
                out[key] = self._alloc_out(rows, n_out, key) if want else None
            rng = Rng(int(seed), int(row0), int(stream_id) & 0xFFFFFFFF, int(step) & 0xFFFFFFFF)
            fn = self.lib.kurbm_half_step_vh_dbg if direction == "vh" else self.lib.kurbm_half_step_hv_dbg
            ld_out = next((m.ld for m in out.values() if m is not None), round_up(n_out, 4))
            check(fn(self.ctx.handle, C.byref(self.params), x.ptr(row_start), rows, x.ld, act, noise,
                     C.byref(rng), out["sample"].ptr() if want_sample else None,
                     out["prob"].ptr() if want_prob else None, out["u"].ptr() if want_u else None,
                     ld_out, self._stream()))
        return out

    def _x3_pieces(self, v, v_chain, mode):
        """Pieces per element of the batch (and of the persistent chain) on the x3 path: 1 when every value is exactly a
        bf16 value, else 3.  The data matrix is looked at once.  The chain is REWRITTEN by every step -- 0/1 states in
        Bernoulli mode, real-valued N(loc, 1) draws in Gaussian mode (rbm.py:64-66) -- so nothing is cached for it beyond
        what the library itself is known to have written there."""
        vp = self.v_pieces(v)
        if v_chain is not None and vp == 1:
            vp = 3 if mode == MODE_VISIBLE_GAUSSIAN else self.v_pieces(v_chain)
        if vp == 1 and v.binary and (v_chain is None or v_chain.binary):
            vp |= _lib.V_BINARY   # 0/1 data (and chain): byte / fp8 planes (include/kurbm.h)
        return vp

    def make_planes(self, v, windows, mode=MODE_VISIBLE_BERNOULLI, v_chain=None):
        """ResidentPlanes of `windows` = [(row_start, rows), ...] of DeviceMatrix v for the x3 steps of a fit(), or None
        when they would not fit comfortably in the free HBM (the steps then convert their rows themselves)."""
        with torch.cuda.device(self.device):
            vp = self._x3_pieces(v, v_chain, mode)
            max_rows = max([rows for _, rows in windows] + [1])
            need = len(windows) * int(self.lib.kurbm_x3_planes_bytes(self.ctx.handle, max_rows, self.n_vis, vp))
            free, _ = torch.cuda.mem_get_info(self.device)
            if need == 0 or need > free // 2:
                return None
            return ResidentPlanes(self, v, windows, vp)

    def _chain_written(self, v_chain, mode):
        if v_chain is not None:
            v_chain.bf16_exact = True if mode == MODE_VISIBLE_BERNOULLI else None
            v_chain.binary = v_chain.bf16_exact

    def cd_step(self, v, rows, row_start, lr, seed, step, k=1, mode=MODE_VISIBLE_BERNOULLI, chain=0,
                which=WHICH_ALL, apply=True, emit_delta=False, v_chain=None, row0=0, v_chain_row=0, bf16=False,
                compute=None, planes=None, momentum=None, n_labels=0):
        """One CD-k update on rows [row_start, row_start+rows) of DeviceMatrix v.

        n_labels > 0: the last n_labels visible units are a softmax label block (kurbm_cd_step_labels; 'fp32' only).

        compute: 'fp32' (fp32 MFMA), 'x3' (fp32 values as exact bf16 triples on the bf16 MFMA),
        'bf16' (operands rounded to bf16).  planes: ResidentPlanes holding these rows (x3: no per-step conversion).
        momentum: None (the reference's bare rule, on the plain entry points) or (mu, weight_decay) -- the update goes through this
        engine's velocity inside the same launch (the *_mom entry points; see _mom for the rule and the scale of weight_decay).
        The one-launch 'small' step has no momentum."""
        compute = compute or ("bf16" if bf16 else "fp32")
        if momentum is not None and compute == "small":
            raise ValueError("the one-launch 'small' step has no momentum: use 'fp32', 'x3' or 'bf16'")
        if n_labels:
            # softmax label units (kurbm_cd_step_labels): the fp32 launches plus the label site behind every h -> v half step
            if compute != "fp32":
                raise ValueError("a label RBM trains on the 'fp32' path only, got %r" % (compute,))
            with torch.cuda.device(self.device):
                opts = CdOpts(int(k), int(mode), float(lr), 1 if apply else 0,
                              self.delta_buffer().data_ptr() if emit_delta else None,
                              v_chain.ptr(v_chain_row) if v_chain is not None else None,
                              int(seed), int(row0), int(step) & 0xFFFFFFFF, int(chain))
                ws = self.workspace(rows, k, v.ld)
                check(self.lib.kurbm_cd_step_labels(self.ctx.handle, C.byref(self.params), int(n_labels), v.ptr(row_start), rows, v.ld,
                                                    C.byref(opts), int(which), ws.data_ptr(), ws.numel(), self._stream(),
                                                    C.byref(self._mom(momentum)) if momentum is not None else None))
            if apply and (which & 1):
                self._weights_written()
            self._chain_written(v_chain, mode)
            return
        # (the plain calls stay as they were, argument for argument: this is the step loop's host path)
        with torch.cuda.device(self.device):
            opts = CdOpts(int(k), int(mode), float(lr), 1 if apply else 0,
                          self.delta_buffer().data_ptr() if emit_delta else None,
                          v_chain.ptr(v_chain_row) if v_chain is not None else None,
                          int(seed), int(row0), int(step) & 0xFFFFFFFF, int(chain))
            if compute == "bf16":
                mir, ws = self.mirror(1), self.workspace_bf16(rows, k)
                if momentum is None:
                    check(self.lib.kurbm_cd_step_bf16(self.ctx.handle, C.byref(self.params), mir.data_ptr(), mir.numel(),
                                                      v.ptr(row_start), rows, v.ld, C.byref(opts), int(which),
                                                      ws.data_ptr(), ws.numel(), self._stream()))
                else:
                    check(self.lib.kurbm_cd_step_bf16_mom(self.ctx.handle, C.byref(self.params), mir.data_ptr(), mir.numel(),
                                                          v.ptr(row_start), rows, v.ld, C.byref(opts), int(which),
                                                          ws.data_ptr(), ws.numel(), self._stream(), C.byref(self._mom(momentum))))
                if apply and (which & 1):
                    self._weights_written(kept=1)
            elif compute == "x3":
                vp = self._x3_pieces(v, v_chain, mode)
                mir, ws = self.mirror(3), self.workspace_bf16(rows, k, 3, vp)
                if planes is not None:
                    opts.v_planes = planes.ptr(v, row_start, rows, vp)
                if momentum is None:
                    check(self.lib.kurbm_cd_step_x3(self.ctx.handle, C.byref(self.params), mir.data_ptr(), mir.numel(),
                                                    v.ptr(row_start), vp, rows, v.ld, C.byref(opts), int(which),
                                                    ws.data_ptr(), ws.numel(), self._stream()))
                else:
                    check(self.lib.kurbm_cd_step_x3_mom(self.ctx.handle, C.byref(self.params), mir.data_ptr(), mir.numel(),
                                                        v.ptr(row_start), vp, rows, v.ld, C.byref(opts), int(which),
                                                        ws.data_ptr(), ws.numel(), self._stream(), C.byref(self._mom(momentum))))
                if apply and (which & 1):
                    self._weights_written(kept=3)
            elif compute == "fp32":
                ws = self.workspace(rows, k, v.ld)
                if momentum is None:
                    check(self.lib.kurbm_cd_step(self.ctx.handle, C.byref(self.params), v.ptr(row_start), rows, v.ld,
                                                 C.byref(opts), int(which), ws.data_ptr(), ws.numel(), self._stream()))
                else:
                    check(self.lib.kurbm_cd_step_mom(self.ctx.handle, C.byref(self.params), v.ptr(row_start), rows, v.ld,
                                                     C.byref(opts), int(which), ws.data_ptr(), ws.numel(), self._stream(),
                                                     C.byref(self._mom(momentum))))
                if apply and (which & 1):
                    self._weights_written()
            elif compute == "small":
                # the whole CD-1 step in one launch (kurbm_small.hip): small problems, where the step is launch latencies
                ws = self.workspace(rows, k)
                check(self.lib.kurbm_cd_step_small(self.ctx.handle, C.byref(self.params), v.ptr(row_start), rows, v.ld,
                                                   C.byref(opts), int(which), ws.data_ptr(), ws.numel(), self._stream()))
                if which & 1:
                    self._weights_written()
            else:
                raise ValueError("compute must be 'fp32', 'x3', 'bf16' or 'small', got %r" % (compute,))
        self._chain_written(v_chain, mode)

    def cd_step_dp(self, comm, v, rows, row_start, lr, seed, step, k=1, mode=MODE_VISIBLE_BERNOULLI, chain=0, row0=0,
                   v_chain=None, v_chain_row=0, compute="x3", n_chunks=0, planes=None, momentum=None):
        """One data-parallel CD-k update: this rank's chain on rows [row_start, +rows) of v (`row0` = their index in
        the global batch), the packed sums all-reduced over `comm` (dp.Comm), the summed update applied.  rows may be 0
        (a rank without rows of a remainder batch still joins the all-reduce).  On the x3 and rounded-bf16 paths all of it
        is ONE library call (kurbm_cd_step_x3_dp / _bf16_dp): one all-reduce of the packed sums on the launch stream (n_chunks > 1
        or KURBM_DP_CHUNKS > 1 opts into row ranges of dW, range i all-reduced + applied on the library's comm stream under the
        statistics GEMM of range i + 1); the fp32-MFMA path runs emit -> kurbm_allreduce_sum_f32 -> apply.
        momentum (see cd_step): every exchange then runs that generic sequence, its apply through the velocity
        (kurbm_apply_delta_mom / kurbm_x3_apply_delta_mom); the summed delta is the same on all ranks, so are the velocities."""
        if momentum is not None:
            delta = self.delta_buffer()
            if rows > 0:
                self.cd_step(v, rows, row_start, lr, seed, step, k=k, mode=mode, chain=chain, apply=False, emit_delta=True,
                             v_chain=v_chain, row0=row0, v_chain_row=v_chain_row, compute=compute, planes=planes)
            else:
                delta.zero_()
            comm.allreduce_sum_(delta)
            self.apply_delta(lr, compute=compute, momentum=momentum)
            return
        if hasattr(comm, "capacity") and compute == "x3":
            # the peer exchange (dp.PeerExchange): chain, statistics, two-shot exchange with the apply fused into its second shot
            with torch.cuda.device(self.device):
                vp = self._x3_pieces(v, v_chain, mode)
                mir, ws = self.mirror(3), self.workspace_bf16(max(rows, 1), k, 3, vp)
                opts = CdOpts(int(k), int(mode), float(lr), 1, None, v_chain.ptr(v_chain_row) if v_chain is not None else None,
                              int(seed), int(row0), int(step) & 0xFFFFFFFF, int(chain))
                if planes is not None and rows > 0:
                    opts.v_planes = planes.ptr(v, row_start, rows, vp)
                check(self.lib.kurbm_cd_step_x3_peer(self.ctx.handle, comm.handle, C.byref(self.params), mir.data_ptr(), mir.numel(),
                                                     v.ptr(row_start), vp, int(rows), v.ld, C.byref(opts), ws.data_ptr(), ws.numel(),
                                                     self._stream()))
            self._weights_written(kept=3)
            self._mirrors[3][1] = False
            if rows > 0:
                self._chain_written(v_chain, mode)
            return
        delta = self.delta_buffer()
        # n_chunks 0: the library's choice (by the size of the exchange; ctx knob KURBM_DP_CHUNKS overrides)
        if compute in ("x3", "bf16") and not hasattr(comm, "capacity"):
            pieces = 3 if compute == "x3" else 1
            with torch.cuda.device(self.device):
                vp = self._x3_pieces(v, v_chain, mode) if pieces == 3 else 1
                mir, ws = self.mirror(pieces), self.workspace_bf16(max(rows, 1), k, pieces, vp)
                opts = CdOpts(int(k), int(mode), float(lr), 1, delta.data_ptr(),
                              v_chain.ptr(v_chain_row) if v_chain is not None else None,
                              int(seed), int(row0), int(step) & 0xFFFFFFFF, int(chain))
                if planes is not None and rows > 0 and pieces == 3:
                    opts.v_planes = planes.ptr(v, row_start, rows, vp)
                if pieces == 3:
                    check(self.lib.kurbm_cd_step_x3_dp(self.ctx.handle, comm.handle, C.byref(self.params), mir.data_ptr(),
                                                       mir.numel(), v.ptr(row_start), vp, int(rows), v.ld, C.byref(opts),
                                                       int(n_chunks), ws.data_ptr(), ws.numel(), self._stream()))
                else:
                    check(self.lib.kurbm_cd_step_bf16_dp(self.ctx.handle, comm.handle, C.byref(self.params), mir.data_ptr(),
                                                         mir.numel(), v.ptr(row_start), int(rows), v.ld, C.byref(opts),
                                                         int(n_chunks), ws.data_ptr(), ws.numel(), self._stream()))
            self._weights_written(kept=pieces)
            self._mirrors[pieces][1] = False
            if rows > 0:
                self._chain_written(v_chain, mode)
            return
        if rows > 0:
            self.cd_step(v, rows, row_start, lr, seed, step, k=k, mode=mode, chain=chain, apply=False, emit_delta=True,
                         v_chain=v_chain, row0=row0, v_chain_row=v_chain_row, compute=compute)
        else:
            delta.zero_()
        comm.allreduce_sum_(delta)
        self.apply_delta(lr, compute=compute)

    def cd_step_x3_stage(self, v, rows, row_start, lr, seed, step, stage, mode=MODE_VISIBLE_BERNOULLI, planes=None):
        """Measurement hook (bench.py, tools/stage_times.py): ONE launch of the x3 CD-1 sequence on the planes the previous
        complete x3 step (same rows, data and mode) left in the workspace; stage numbering as kurbm_cd_step_x3_stage."""
        with torch.cuda.device(self.device):
            vp = self._x3_pieces(v, None, mode)   # (as cd_step passes it: the planes must read the same)
            mir, ws = self.mirror(3), self.workspace_bf16(rows, 1, 3, vp)
            opts = CdOpts(1, int(mode), float(lr), 1, None, None, int(seed), 0, int(step) & 0xFFFFFFFF, 0)
            if planes is not None:
                opts.v_planes = planes.ptr(v, row_start, rows, vp)
            check(self.lib.kurbm_cd_step_x3_stage(self.ctx.handle, C.byref(self.params), mir.data_ptr(), mir.numel(),
                                                  v.ptr(row_start), vp, rows, v.ld, C.byref(opts), WHICH_ALL, int(stage),
                                                  ws.data_ptr(), ws.numel(), self._stream()))
            if stage == 5:
                self._weights_written(kept=3)

    def cd_epoch(self, v, n_rows, batch_size, lr, seed, step0, k=1, mode=MODE_VISIBLE_BERNOULLI, v_chain=None,
                 compute="fp32", row_start=0, planes=None, momentum=None, n_labels=0):
        """All batches of rows [row_start, row_start + n_rows) in ONE library call (fused updates, no score); returns #steps.
        momentum (see cd_step): one (mu, weight_decay) for the whole call.  n_labels > 0: kurbm_cd_epoch_labels ('fp32' only)."""
        if momentum is not None and compute == "small":
            raise ValueError("the one-launch 'small' step has no momentum: use 'fp32' or 'x3'")
        if n_labels:
            if compute != "fp32":
                raise ValueError("a label RBM trains on the 'fp32' path only, got %r" % (compute,))
            with torch.cuda.device(self.device):
                ws = self.workspace(min(batch_size, max(n_rows, 1)), k, v.ld)
                opts = CdOpts(int(k), int(mode), float(lr), 1, None, v_chain.ptr() if v_chain is not None else None,
                              int(seed), 0, int(step0) & 0xFFFFFFFF, 0)
                n = self.lib.kurbm_cd_epoch_labels(self.ctx.handle, C.byref(self.params), int(n_labels), v.ptr(row_start), int(n_rows),
                                                   v.ld, int(batch_size), C.byref(opts), ws.data_ptr(), ws.numel(), self._stream(),
                                                   C.byref(self._mom(momentum)) if momentum is not None else None)
                if n < 0:
                    check(n)
            self._weights_written()
            self._chain_written(v_chain, mode)
            return n
        mom = ()
        if momentum is not None:
            with torch.cuda.device(self.device):
                mom = (C.byref(self._mom(momentum)),)
        if compute == "x3":
            with torch.cuda.device(self.device):
                vp = self._x3_pieces(v, v_chain, mode)
                rows = min(batch_size, max(n_rows, 1))
                mir, ws = self.mirror(3), self.workspace_bf16(rows, k, 3, vp)
                opts = CdOpts(int(k), int(mode), float(lr), 1, None, v_chain.ptr() if v_chain is not None else None,
                              int(seed), 0, int(step0) & 0xFFFFFFFF, 0)
                if planes is not None and planes.v is v and planes.v_pieces == vp and planes.uniform(row_start, n_rows, batch_size):
                    opts.v_planes, opts.v_planes_stride = planes.buf.data_ptr(), planes.stride
                fn = self.lib.kurbm_cd_epoch_x3_mom if mom else self.lib.kurbm_cd_epoch_x3
                n = fn(self.ctx.handle, C.byref(self.params), mir.data_ptr(), mir.numel(), v.ptr(row_start), vp,
                       int(n_rows), v.ld, int(batch_size), C.byref(opts), ws.data_ptr(), ws.numel(),
                       self._stream(), *mom)
                if n < 0:
                    check(n)
            self._weights_written(kept=3)
            self._chain_written(v_chain, mode)
            return n
        with torch.cuda.device(self.device):
            ws = self.workspace(min(batch_size, max(n_rows, 1)), k, 0 if compute == "small" else v.ld)
            opts = CdOpts(int(k), int(mode), float(lr), 1, None, v_chain.ptr() if v_chain is not None else None,
                          int(seed), 0, int(step0) & 0xFFFFFFFF, 0)
            fn = self.lib.kurbm_cd_epoch_small if compute == "small" else (self.lib.kurbm_cd_epoch_mom if mom else self.lib.kurbm_cd_epoch)
            n = fn(self.ctx.handle, C.byref(self.params), v.ptr(row_start), int(n_rows), v.ld,
                                        int(batch_size), C.byref(opts), ws.data_ptr(), ws.numel(), self._stream(), *mom)
            if n < 0:
                check(n)
        self._weights_written()
        self._chain_written(v_chain, mode)
        return n

    def cd_epoch_small_scored(self, v, n_rows, batch_size, lr, seed, step0, mode, score_chain, row_start=0):
        """The batch loop of fit(verbose=1) for a small RBM as ONE library call (kurbm_cd_epoch_small_scored): every batch's
        one-launch update followed by its one-launch score.  Returns (#steps, scores): scores is a PINNED host tensor
        [steps, 2] that the device fills as it goes -- scores[i, 0] the score of step i, scores[i, 1] turning 1.0 when it has
        landed -- so the caller prints the lines while the device runs on, without synchronising."""
        steps = -(-int(n_rows) // int(batch_size)) if n_rows > 0 else 0
        scores = torch.zeros((max(steps, 1), 2), dtype=torch.float32, pin_memory=True)
        with torch.cuda.device(self.device):
            ws = self.workspace(min(batch_size, max(n_rows, 1)))
            opts = CdOpts(1, int(mode), float(lr), 1, None, None, int(seed), 0, int(step0) & 0xFFFFFFFF, 0)
            n = self.lib.kurbm_cd_epoch_small_scored(self.ctx.handle, C.byref(self.params), v.ptr(row_start), int(n_rows), v.ld,
                                                     int(batch_size), C.byref(opts), int(score_chain), scores.data_ptr(),
                                                     ws.data_ptr(), ws.numel(), self._stream())
            if n < 0:
                check(n)
        self._weights_written()
        return n, scores

    def half_step_bf16(self, direction, x, rows, act, noise, seed, stream_id, step, row0=0, pieces=1, row_start=0,
                       want_prob=True, want_u=True, in_format=None):
        """One half step with bf16 products (pieces=3: the exact split, used by transform() on the x3 path; pieces=1:
        rounded operands, a test hook); fp32 planes (sample, prob, u) as requested.
        in_format (pieces=3 only) forces how the input is staged: 'bytes' (the caller promises 0/1 values: the byte plane of the
        steps' 0/1 data and samples), 'bf16' (one piece: every value exactly bf16) or 'x3' (three pieces: always legal).
        None: one piece if x is exactly bf16, else three."""
        n_out = self.n_hid if direction == "vh" else self.n_vis
        if in_format is not None and (pieces != 3 or in_format not in ("bytes", "bf16", "x3")):
            raise ValueError("in_format is 'bytes', 'bf16' or 'x3', with pieces=3; got %r with pieces=%d" % (in_format, pieces))
        with torch.cuda.device(self.device):
            if in_format is not None:
                xp = {"bytes": 1 | _lib.V_BINARY, "bf16": 1, "x3": 3}[in_format]
            else:
                xp = self.v_pieces(x) if pieces == 3 else 1
            mir, ws = self.mirror(pieces), self.workspace_bf16(rows, 1, pieces, xp if pieces == 3 else 1)
            want = {"sample": bool(noise), "prob": bool(want_prob) or not noise, "u": bool(want_u) and bool(noise)}
            out = {k: (self._alloc_out(rows, n_out, k) if want[k] else None) for k in ("sample", "prob", "u")}
            rng = Rng(int(seed), int(row0), int(stream_id) & 0xFFFFFFFF, int(step) & 0xFFFFFFFF)
            tail = (act, noise, C.byref(rng), out["sample"].ptr() if out["sample"] is not None else None,
                    out["prob"].ptr() if out["prob"] is not None else None, out["u"].ptr() if out["u"] is not None else None,
                    next((m.ld for m in out.values() if m is not None), round_up(n_out, 4)), ws.data_ptr(), ws.numel(),
                    self._stream())
            d = 0 if direction == "vh" else 1
            if pieces == 3:
                check(self.lib.kurbm_half_step_x3(self.ctx.handle, C.byref(self.params), mir.data_ptr(), mir.numel(), d,
                                                  x.ptr(row_start), xp, rows, x.ld, *tail))
            else:
                check(self.lib.kurbm_half_step_bf16(self.ctx.handle, C.byref(self.params), mir.data_ptr(), mir.numel(), d,
                                                    x.ptr(row_start), rows, x.ld, *tail))
            if noise == NOISE_BERNOULLI and out["sample"] is not None:
                out["sample"].bf16_exact = out["sample"].binary = True        # 0/1: one bf16 piece, no need to look
            elif noise == NOISE_GAUSSIAN and out["sample"] is not None:
                out["sample"].bf16_exact = out["sample"].binary = False
        return out

    def apply_delta(self, lr, which=WHICH_ALL, delta=None, compute=None, momentum=None):
        """W, b_h, b_v += lr * delta (the all-reduced packed sums).  compute='x3' also rewrites the weight-piece
        mirror in the same launch.  momentum (see cd_step): the same update through the velocity."""
        delta = self.delta_buffer() if delta is None else delta
        with torch.cuda.device(self.device):
            mom = (C.byref(self._mom(momentum)),) if momentum is not None else ()
            if compute == "x3" and 3 in self._mirrors:
                mir = self._mirrors[3][0]
                fn = self.lib.kurbm_x3_apply_delta_mom if mom else self.lib.kurbm_x3_apply_delta
                check(fn(self.ctx.handle, C.byref(self.params), mir.data_ptr(), mir.numel(),
                         delta.data_ptr(), float(lr), int(which), self._stream(), *mom))
                self._weights_written(kept=3)
                self._mirrors[3][1] = False
                return
            fn = self.lib.kurbm_apply_delta_mom if mom else self.lib.kurbm_apply_delta
            check(fn(self.ctx.handle, C.byref(self.params), delta.data_ptr(), float(lr),
                     int(which), self._stream(), *mom))
        self._weights_written()

    def free_energy(self, v, rows, row_start=0, compute=None):
        """F(v) per row (rbm.py:73-76).  compute='x3': the v.W product on the bf16 pieces (fp32-equivalent)."""
        with torch.cuda.device(self.device):
            F = self._alloc_floats(rows, "F", zero=False)
            if compute == "x3":
                vp = self.v_pieces(v)
                mir, ws = self.mirror(3), self.workspace_bf16(rows, 1, 3, vp)
                check(self.lib.kurbm_free_energy_x3(self.ctx.handle, C.byref(self.params), mir.data_ptr(), mir.numel(),
                                                    v.ptr(row_start), vp, rows, v.ld, F.data_ptr(), ws.data_ptr(),
                                                    ws.numel(), self._stream()))
                return F
            ws = self.workspace(rows)
            check(self.lib.kurbm_free_energy(self.ctx.handle, C.byref(self.params), v.ptr(row_start), rows, v.ld,
                                             F.data_ptr(), ws.data_ptr(), ws.numel(), self._stream()))
        return F

    # -- annealed importance sampling (include/kurbm.h: kurbm_ais_run) --------------------------
    def ais_workspace(self, n_chains, n_labels=0):
        if n_labels:
            n = int(self.lib.kurbm_ais_labels_workspace_bytes(self.ctx.handle, int(n_chains), self.n_vis, self.n_hid, int(n_labels)))
        else:
            n = int(self.lib.kurbm_ais_workspace_bytes(self.ctx.handle, int(n_chains), self.n_vis, self.n_hid))
        if n == 0:
            raise _lib.KurbmError("kurbm_ais%s_workspace_bytes failed" % ("_labels" if n_labels else ""))
        return self._alloc_bytes(n, "ais_workspace", zero=False)

    def _base_bias(self, base_bias):
        """b_A [n_vis] on the device: a device tensor as is, a host array uploaded, None = zeros (the uniform base model)."""
        if isinstance(base_bias, torch.Tensor) and base_bias.device == self.device:
            if base_bias.dtype != torch.float32 or base_bias.numel() != self.n_vis:
                raise ValueError("base_bias must hold %d fp32 values" % self.n_vis)
            return base_bias
        b = np.zeros(self.n_vis, np.float32) if base_bias is None else np.ascontiguousarray(base_bias, dtype=np.float32).reshape(-1)
        if b.size != self.n_vis:
            raise ValueError("base_bias has %d values, the RBM has %d visible units" % (b.size, self.n_vis))
        t = self._alloc_floats(self.n_vis, "base_bias", zero=False)
        t.copy_(torch.from_numpy(b))
        return t

    def ais_run(self, betas, n_chains, base_bias=None, chain0=0, seed=0, want_v=False, ws=None, n_labels=0):
        """log w of n_chains AIS chains (global indices chain0 ...) over the schedule `betas` (host float64, 0 .. 1, strictly
        increasing) in ONE library call: two GEMM launches and one small launch per temperature, nothing read back here.
        n_labels > 0: the last n_labels visible units are a softmax label block (kurbm_ais_run_labels: one more small launch per
        temperature).  Returns (logw: float64 device tensor [n_chains], v_final: DeviceMatrix or None)."""
        betas = np.ascontiguousarray(betas, dtype=np.float64).reshape(-1)
        n_chains, n_labels = int(n_chains), int(n_labels)
        with torch.cuda.device(self.device):
            ba = self._base_bias(base_bias)
            ws = self.ais_workspace(n_chains, n_labels) if ws is None else ws
            logw = self._alloc_floats(2 * n_chains, "logw", zero=False).view(torch.float64)
            vf = self._alloc_out(n_chains, self.n_vis, "v_final") if want_v else None
            tail = (betas.ctypes.data_as(C.POINTER(C.c_double)), int(betas.size), n_chains, int(chain0), int(seed), logw.data_ptr(),
                    vf.ptr() if want_v else None, vf.ld if want_v else 0, ws.data_ptr(), ws.numel(), self._stream())
            if n_labels:
                check(self.lib.kurbm_ais_run_labels(self.ctx.handle, C.byref(self.params), n_labels, ba.data_ptr(), *tail))
            else:
                check(self.lib.kurbm_ais_run(self.ctx.handle, C.byref(self.params), ba.data_ptr(), *tail))
        return logw, vf

    def ais_step_labels(self, v, n_labels, beta_prev, beta, k, base_bias=None, chain0=0, seed=0, want_planes=True, ws=None):
        """Test hook: ais_step for a label RBM (kurbm_ais_step_labels); v carries a one-hot block.  The dict of ais_step plus,
        with want_planes, prob_y (DeviceMatrix [rows, n_labels]) and u_y (device tensor [rows])."""
        if v.cols != self.n_vis:
            raise ValueError("input has %d columns, expected %d" % (v.cols, self.n_vis))
        rows, n_labels = v.rows, int(n_labels)
        with torch.cuda.device(self.device):
            ba = self._base_bias(base_bias)
            ws = self.ais_workspace(rows, n_labels) if ws is None else ws
            out = {"dlogw": self._alloc_floats(rows, "dlogw", zero=False)}
            for key, cols, want in (("h", self.n_hid, True), ("prob_h", self.n_hid, want_planes), ("u_h", self.n_hid, want_planes),
                                    ("v", self.n_vis, True), ("prob_v", self.n_vis, want_planes), ("u_v", self.n_vis, want_planes),
                                    ("prob_y", n_labels, want_planes)):
                out[key] = self._alloc_out(rows, cols, key) if want else None
            out["u_y"] = self._alloc_floats(rows, "u_y", zero=False) if want_planes else None
            ptr = lambda key: out[key].ptr() if out[key] is not None else None
            check(self.lib.kurbm_ais_step_labels(self.ctx.handle, C.byref(self.params), n_labels, ba.data_ptr(), float(beta_prev),
                                                 float(beta), int(k), v.ptr(), v.ld, rows, int(chain0), int(seed),
                                                 out["dlogw"].data_ptr(), ptr("h"), out["h"].ld, ptr("v"), out["v"].ld, ptr("prob_h"),
                                                 ptr("u_h"), ptr("prob_v"), ptr("u_v"), ptr("prob_y"),
                                                 out["prob_y"].ld if want_planes else 0,
                                                 out["u_y"].data_ptr() if want_planes else None, ws.data_ptr(), ws.numel(),
                                                 self._stream()))
        return out

    def ais_step(self, v, beta_prev, beta, k, base_bias=None, chain0=0, seed=0, want_planes=True, ws=None):
        """Test hook: temperature k of such a run on the chains in DeviceMatrix v (kurbm_ais_step, teacher-forced).  Returns a
        dict: dlogw (fp32 device tensor), h, v (DeviceMatrix) and, with want_planes, prob_h, u_h, prob_v, u_v."""
        if v.cols != self.n_vis:
            raise ValueError("input has %d columns, expected %d" % (v.cols, self.n_vis))
        rows = v.rows
        with torch.cuda.device(self.device):
            ba = self._base_bias(base_bias)
            ws = self.ais_workspace(rows) if ws is None else ws
            out = {"dlogw": self._alloc_floats(rows, "dlogw", zero=False)}
            for key, cols, want in (("h", self.n_hid, True), ("prob_h", self.n_hid, want_planes), ("u_h", self.n_hid, want_planes),
                                    ("v", self.n_vis, True), ("prob_v", self.n_vis, want_planes), ("u_v", self.n_vis, want_planes)):
                out[key] = self._alloc_out(rows, cols, key) if want else None
            ptr = lambda key: out[key].ptr() if out[key] is not None else None
            check(self.lib.kurbm_ais_step(self.ctx.handle, C.byref(self.params), ba.data_ptr(), float(beta_prev), float(beta), int(k),
                                          v.ptr(), v.ld, rows, int(chain0), int(seed), out["dlogw"].data_ptr(),
                                          ptr("h"), out["h"].ld, ptr("v"), out["v"].ld, ptr("prob_h"), ptr("u_h"), ptr("prob_v"),
                                          ptr("u_v"), ws.data_ptr(), ws.numel(), self._stream()))
        return out

    # -- Gibbs runs (include/kurbm.h: kurbm_gibbs_run) ------------------------------------------
    def gibbs_workspace(self, n_chains, v_pieces, mode):
        n = int(self.lib.kurbm_gibbs_workspace_bytes(self.ctx.handle, int(n_chains), self.n_vis, self.n_hid, int(v_pieces), int(mode)))
        if n == 0:
            raise _lib.KurbmError("kurbm_gibbs_workspace_bytes failed")
        return self._alloc_bytes(n, "gibbs_workspace", zero=False)

    def _clamp_mask(self, clamp):
        """The clamp mask as n_vis device bytes (non-zero = clamped): a uint8 device tensor as is; a boolean mask [n_vis] or a
        list of unit indices uploaded; None stays None."""
        if clamp is None:
            return None
        if isinstance(clamp, torch.Tensor) and clamp.dtype == torch.uint8 and clamp.device == self.device:
            if clamp.numel() != self.n_vis:
                raise ValueError("clamp has %d entries, the RBM has %d visible units" % (clamp.numel(), self.n_vis))
            return clamp
        t = self._alloc_bytes(self.n_vis, "clamp", zero=False)
        t.copy_(torch.from_numpy(clamp_mask(clamp, self.n_vis)))
        return t

    def gibbs_run(self, v, burn_in=1, thin=1, n_keep=1, chain0=0, seed=0, mode=MODE_VISIBLE_BERNOULLI, clamp=None,
                  want_prob=False, ws=None, n_labels=0):
        """Gibbs sweeps from the rows of DeviceMatrix v (one chain per row, global indices chain0 ...) in ONE library call: two
        x3 half-step launches per sweep, the states kept in their operand format, nothing read back here.  Kept sample j is the
        state after burn_in + j * thin sweeps.  clamp: see _clamp_mask; those units keep v's values.
        n_labels > 0: the last n_labels visible units are a FREE softmax label block, drawn by the label site every sweep
        (kurbm_gibbs_run_labels: one more small launch per sweep); the block's entries of clamp are not read.
        Returns (samples, probs): DeviceMatrix [n_keep * rows, n_vis] in (kept, chain) order; probs (want_prob, else None) holds
        the activated value each sample was drawn from."""
        if v.cols != self.n_vis:
            raise ValueError("input has %d columns, expected %d" % (v.cols, self.n_vis))
        rows, n_keep = int(v.rows), int(n_keep)
        if rows < 1:
            raise ValueError("a Gibbs run needs at least one chain")
        with torch.cuda.device(self.device):
            vp = self._x3_pieces(v, None, mode)
            mask = self._clamp_mask(clamp)
            mir = self.mirror(3)
            ws = self.gibbs_workspace(rows, vp, mode) if ws is None else ws
            out = self._alloc_out(max(n_keep, 1) * rows, self.n_vis, "gibbs_v")
            prob = self._alloc_out(max(n_keep, 1) * rows, self.n_vis, "gibbs_prob") if want_prob else None
            tail = (mir.data_ptr(), mir.numel(), v.ptr(), vp, v.ld, rows, int(chain0), int(seed), int(mode), int(burn_in), int(thin),
                    n_keep, mask.data_ptr() if mask is not None else None, out.ptr(), prob.ptr() if prob is not None else None,
                    out.ld, rows * out.ld, ws.data_ptr(), ws.numel(), self._stream())
            if n_labels:
                check(self.lib.kurbm_gibbs_run_labels(self.ctx.handle, C.byref(self.params), int(n_labels), *tail))
            else:
                check(self.lib.kurbm_gibbs_run(self.ctx.handle, C.byref(self.params), *tail))
            if mode == MODE_VISIBLE_BERNOULLI and mask is None:
                out.bf16_exact = out.binary = True        # 0/1: one bf16 piece, no need to look
        return out, prob

    # -- softmax label units (include/kurbm.h: kurbm_label_sample, kurbm_class_logits) ----------
    def label_sample(self, h, v, n_labels, seed, stream_id, step, row0=0, want_prob=False, want_u=False):
        """The label site alone: the last n_labels columns of DeviceMatrix v [rows, n_vis] are REWRITTEN in place as the one-hot
        draw from softmax(b_v + h.W^T) of the rows of DeviceMatrix h [rows, n_hid]; one uniform per row, u(row0 + row, n_pix) at
        (stream_id, step).  Returns a dict: prob (DeviceMatrix [rows, n_labels]) and u (device tensor [rows]) as requested."""
        if h.cols != self.n_hid or v.cols != self.n_vis or h.rows != v.rows:
            raise ValueError("label_sample: h is (%d, %d), v is (%d, %d); the RBM is %d x %d"
                             % (h.rows, h.cols, v.rows, v.cols, self.n_vis, self.n_hid))
        rows = h.rows
        with torch.cuda.device(self.device):
            prob = self._alloc_out(rows, int(n_labels), "label_prob") if want_prob else None
            u = self._alloc_floats(rows, "label_u", zero=False) if want_u else None
            rng = Rng(int(seed), int(row0), int(stream_id) & 0xFFFFFFFF, int(step) & 0xFFFFFFFF)
            check(self.lib.kurbm_label_sample(self.ctx.handle, C.byref(self.params), int(n_labels), h.ptr(), rows, h.ld, C.byref(rng),
                                              v.ptr(), v.ld, prob.ptr() if want_prob else None, prob.ld if want_prob else 0,
                                              u.data_ptr() if want_u else None, self._stream()))
        return {"prob": prob, "u": u}

    def class_workspace(self, rows):
        n = int(self.lib.kurbm_class_workspace_bytes(self.ctx.handle, int(rows), self.n_vis, self.n_hid))
        if n == 0:
            raise _lib.KurbmError("kurbm_class_workspace_bytes failed")
        return self._alloc_bytes(n, "class_workspace", zero=False)

    def class_logits(self, v, n_labels, rows=None, row_start=0, want_prob=True, ws=None):
        """(logits, prob): DeviceMatrix [rows, n_labels] each (prob None without want_prob) for the pixels of DeviceMatrix v, which
        has n_vis - n_labels columns or n_vis (the label block is ignored).  Two launches (kurbm_class_logits)."""
        n_pix = self.n_vis - int(n_labels)
        if v.cols not in (n_pix, self.n_vis):
            raise ValueError("input has %d columns, expected %d (pixels) or %d (pixels and labels)" % (v.cols, n_pix, self.n_vis))
        rows = v.rows - row_start if rows is None else int(rows)
        with torch.cuda.device(self.device):
            ws = self.class_workspace(rows) if ws is None else ws
            logits = self._alloc_out(rows, int(n_labels), "logits")
            prob = self._alloc_out(rows, int(n_labels), "class_prob") if want_prob else None
            check(self.lib.kurbm_class_logits(self.ctx.handle, C.byref(self.params), int(n_labels), v.ptr(row_start), rows, v.ld,
                                              logits.ptr(), logits.ld, prob.ptr() if want_prob else None, ws.data_ptr(), ws.numel(),
                                              self._stream()))
        return logits, prob

    # -- discriminative / hybrid training of a label RBM (include/kurbm.h: kurbm_disc_step) ------
    def disc_workspace(self, rows, n_labels, ldv=0):
        """Scratch of class_grad / disc_step / disc_epoch for batches of <= rows (kurbm_disc_workspace_bytes).  ldv: the leading
        dimension of the batch of a HYBRID step when it exceeds round_up(n_vis, 4) (the generative chain keeps v_neg at it)."""
        n = int(self.lib.kurbm_disc_workspace_bytes(self.ctx.handle, int(rows), self.n_vis, self.n_hid, int(n_labels)))
        if n == 0:
            raise _lib.KurbmError("kurbm_disc_workspace_bytes failed")
        ldc = round_up(self.n_vis, 4)
        n += round_up(rows * max(int(ldv), ldc) * 4, 256) - round_up(rows * ldc * 4, 256)
        return self._alloc_bytes(n, "disc_workspace", zero=False)

    def _disc_ws(self, rows, n_labels, ldv):
        key = (int(n_labels), max(int(ldv), round_up(self.n_vis, 4)))
        have = self._ws_disc
        if have is None or have[0] != key or rows > have[1]:
            have = self._ws_disc = (key, rows, self.disc_workspace(rows, n_labels, ldv))
        return have[2]

    def class_grad(self, v, n_labels, rows=None, row_start=0, want_planes=True, want_nll=True, ws=None):
        """The discriminative gradient of rows [row_start, +rows) of DeviceMatrix v [*, n_vis] (label block last) as a dict: S_y and
        H_bar (DeviceMatrix [rows, n_hid]; None without want_planes), nll (device tensor [rows]; None without want_nll) and delta,
        the packed [dW | db_h | db_v] sums in this engine's delta buffer.  Nothing is applied (kurbm_class_grad)."""
        if v.cols != self.n_vis:
            raise ValueError("input has %d columns, expected %d (pixels and labels)" % (v.cols, self.n_vis))
        rows = v.rows - row_start if rows is None else int(rows)
        with torch.cuda.device(self.device):
            ws = self.disc_workspace(rows, n_labels) if ws is None else ws
            S_y = self._alloc_out(rows, self.n_hid, "S_y") if want_planes else None
            H_bar = self._alloc_out(rows, self.n_hid, "H_bar") if want_planes else None
            nll = self._alloc_floats(rows, "nll", zero=False) if want_nll else None
            delta = self.delta_buffer()
            check(self.lib.kurbm_class_grad(self.ctx.handle, C.byref(self.params), int(n_labels), v.ptr(row_start), rows, v.ld,
                                            S_y.ptr() if want_planes else None, H_bar.ptr() if want_planes else None,
                                            S_y.ld if want_planes else 0, nll.data_ptr() if want_nll else None, delta.data_ptr(),
                                            ws.data_ptr(), ws.numel(), self._stream()))
        return {"S_y": S_y, "H_bar": H_bar, "nll": nll, "delta": delta}

    def disc_step(self, v, rows, row_start, lr, n_labels, gen_weight=0.0, seed=0, step=0, k=1, chain=0, v_chain=None, row0=0,
                  momentum=None, want_nll=False, ws=None):
        """One discriminative (gen_weight = 0) or hybrid (gen_weight > 0) update on rows [row_start, +rows) of DeviceMatrix v
        (kurbm_disc_step).  seed, step, k, chain, v_chain, row0 are those of the generative chain of a hybrid step; momentum as in
        cd_step.  want_nll: returns a device tensor whose element 0 is the batch's mean nll before the update, else None."""
        with torch.cuda.device(self.device):
            opts = CdOpts(int(k), MODE_VISIBLE_BERNOULLI, float(lr), 1, None, v_chain.ptr() if v_chain is not None else None,
                          int(seed), int(row0), int(step) & 0xFFFFFFFF, int(chain))
            ws = self._disc_ws(rows, n_labels, v.ld) if ws is None else ws
            nll = self._alloc_floats(1, "nll_mean", zero=False) if want_nll else None
            check(self.lib.kurbm_disc_step(self.ctx.handle, C.byref(self.params), int(n_labels), v.ptr(row_start), rows, v.ld,
                                           C.byref(opts), float(gen_weight), nll.data_ptr() if want_nll else None, ws.data_ptr(),
                                           ws.numel(), self._stream(), C.byref(self._mom(momentum)) if momentum is not None else None))
        self._weights_written()
        if gen_weight > 0:
            self._chain_written(v_chain, MODE_VISIBLE_BERNOULLI)
        return nll

    def disc_epoch(self, v, n_rows, batch_size, lr, n_labels, gen_weight=0.0, seed=0, step0=0, k=1, v_chain=None, row_start=0,
                   momentum=None, want_nll=False, ws=None):
        """All batches of rows [row_start, +n_rows) in ONE library call (kurbm_disc_epoch); returns #steps, or with want_nll
        (#steps, device tensor of each batch's mean nll)."""
        with torch.cuda.device(self.device):
            opts = CdOpts(int(k), MODE_VISIBLE_BERNOULLI, float(lr), 1, None, v_chain.ptr() if v_chain is not None else None,
                          int(seed), 0, int(step0) & 0xFFFFFFFF, 0)
            rows = min(int(batch_size), max(int(n_rows), 1))
            ws = self._disc_ws(rows, n_labels, v.ld) if ws is None else ws
            nsteps = (int(n_rows) + int(batch_size) - 1) // int(batch_size)
            nll = self._alloc_floats(max(nsteps, 1), "nll_means", zero=False) if want_nll else None
            n = self.lib.kurbm_disc_epoch(self.ctx.handle, C.byref(self.params), int(n_labels), v.ptr(row_start), int(n_rows), v.ld,
                                          int(batch_size), C.byref(opts), float(gen_weight), nll.data_ptr() if want_nll else None,
                                          ws.data_ptr(), ws.numel(), self._stream(),
                                          C.byref(self._mom(momentum)) if momentum is not None else None)
            if n < 0:
                check(n)
        self._weights_written()
        if gen_weight > 0:
            self._chain_written(v_chain, MODE_VISIBLE_BERNOULLI)
        return (n, nll) if want_nll else n

    # -- fine-tuning a DBN (include/kurbm.h: kurbm_backprop_layer) -------------------------------
    def probs_into(self, x, rows, row_start, act, out, out_row=0):
        """The prob-only v -> h half step of rows [row_start, +rows) of DeviceMatrix x, written into rows [out_row, +rows) of the
        caller's plane `out` at ITS leading dimension (out.cols >= n_hid: the first n_hid columns are written, the rest is left
        alone) -- a lower layer's activations go straight into the pixel columns of the top layer's batch plane.  fp32 MFMA, no draw."""
        if x.cols != self.n_vis or out.cols < self.n_hid:
            raise ValueError("input has %d columns and the plane %d; the RBM is %d x %d" % (x.cols, out.cols, self.n_vis, self.n_hid))
        with torch.cuda.device(self.device):
            check(self.lib.kurbm_half_step_vh(self.ctx.handle, C.byref(self.params), x.ptr(row_start), int(rows), x.ld, int(act),
                                              NOISE_NONE, None, None, out.ptr(out_row), out.ld, self._stream()))
        return out

    def backprop_workspace(self, rows, n_in=None):
        """Scratch of backprop_layer for batches of <= rows (kurbm_backprop_workspace_bytes); n_in = 1: of backprop_delta."""
        n = int(self.lib.kurbm_backprop_workspace_bytes(self.ctx.handle, int(rows), self.n_vis if n_in is None else int(n_in), self.n_hid))
        if n == 0:
            raise _lib.KurbmError("kurbm_backprop_workspace_bytes failed")
        return self._alloc_bytes(n, "backprop_workspace", zero=False)

    def _backprop_ws(self, rows):
        have = self._ws_bp
        if have is None or rows > have[0]:
            have = self._ws_bp = (rows, self.backprop_workspace(rows))
        return have[1]

    def backprop_delta(self, e, x_out, act, rows=None, in_place=False, ws=None):
        """The activation-derivative site alone (kurbm_backprop_delta, test hook): delta = e * act'(x_out) for DeviceMatrix e and
        x_out [rows, n_hid], and db_h = its column sums.  in_place: delta is written over e.  Returns (delta, db_h device tensor)."""
        rows = e.rows if rows is None else int(rows)
        with torch.cuda.device(self.device):
            ws = self.backprop_workspace(rows, 1) if ws is None else ws
            delta = e if in_place else self._alloc_out(rows, self.n_hid, "bp_delta")
            db_h = self._alloc_floats(self.n_hid, "bp_db_h", zero=False)
            check(self.lib.kurbm_backprop_delta(self.ctx.handle, e.ptr(), e.ld, x_out.ptr(), x_out.ld, rows, self.n_hid, int(act),
                                                delta.ptr(), delta.ld, db_h.data_ptr(), ws.data_ptr(), ws.numel(), self._stream()))
        return delta, db_h

    def backprop_layer(self, act, x_in, x_out, e, rows=None, row_start=0, e_in=None, ws=None):
        """This layer's share of a backward pass (kurbm_backprop_layer): x_in rows [row_start, +rows) of a DeviceMatrix [*, n_vis];
        x_out and e the first `rows` rows of DeviceMatrix planes with >= n_hid columns (x_out as probs_into left it; e holds
        dL/dx_out and is OVERWRITTEN with delta); e_in (DeviceMatrix [>= rows, n_vis] or None) receives dL/dx_in.  The packed
        [dW | db_h | db_v = 0] sums land in this engine's delta buffer, which is returned.  Nothing is applied."""
        rows = e.rows if rows is None else int(rows)
        with torch.cuda.device(self.device):
            ws = self._backprop_ws(rows) if ws is None else ws
            delta = self.delta_buffer()
            check(self.lib.kurbm_backprop_layer(self.ctx.handle, C.byref(self.params), int(act), x_in.ptr(row_start), x_in.ld,
                                                x_out.ptr(), x_out.ld, e.ptr(), e.ld, rows, delta.data_ptr(),
                                                e_in.ptr() if e_in is not None else None, e_in.ld if e_in is not None else 0,
                                                ws.data_ptr(), ws.numel(), self._stream()))
        return delta

    def disc_backprop(self, v, n_labels, rows=None, row_start=0, e_in=None, want_nll=False, ws=None):
        """The top label RBM's share (kurbm_disc_backprop): the launches of class_grad on rows [row_start, +rows) of DeviceMatrix v
        [*, n_vis] (label block last) into this engine's delta buffer, then e_in (DeviceMatrix [>= rows, n_pix] or None) =
        g.W[:n_pix]^T.  Nothing is applied.  Returns (delta, nll): nll a device tensor whose element 0 is the batch's mean
        -log p(y | v), or None without want_nll."""
        if v.cols != self.n_vis:
            raise ValueError("input has %d columns, expected %d (pixels and labels)" % (v.cols, self.n_vis))
        rows = v.rows - row_start if rows is None else int(rows)
        with torch.cuda.device(self.device):
            ws = self._disc_ws(rows, n_labels, v.ld) if ws is None else ws
            delta = self.delta_buffer()
            nll = self._alloc_floats(1, "nll_mean", zero=False) if want_nll else None
            check(self.lib.kurbm_disc_backprop(self.ctx.handle, C.byref(self.params), int(n_labels), v.ptr(row_start), rows, v.ld,
                                               delta.data_ptr(), e_in.ptr() if e_in is not None else None,
                                               e_in.ld if e_in is not None else 0, nll.data_ptr() if want_nll else None,
                                               ws.data_ptr(), ws.numel(), self._stream()))
        return delta, nll

    def score_x3(self, v, rows, row_start, seed, step, mode, chain, planes=None):
        """mean |F(v) - F(v')| of rows [row_start, +rows) of v, v' a fresh one-step reconstruction (rbm.py:225-233), in ONE
        library call on the x3 kernels; returns a device tensor whose element 0 is the score -- nothing is read back here."""
        with torch.cuda.device(self.device):
            vp = self._x3_pieces(v, None, mode)
            mir, ws = self.mirror(3), self.workspace_bf16(rows, 1, 3, vp)
            opts = CdOpts(1, int(mode), 0.0, 0, None, None, int(seed), 0, int(step) & 0xFFFFFFFF, int(chain))
            if planes is not None:
                opts.v_planes = planes.ptr(v, row_start, rows, vp)
            out = self._alloc_floats(4, "score", zero=False)
            check(self.lib.kurbm_score_x3(self.ctx.handle, C.byref(self.params), mir.data_ptr(), mir.numel(), v.ptr(row_start), vp,
                                          int(rows), v.ld, C.byref(opts), out.data_ptr(), None, ws.data_ptr(), ws.numel(),
                                          self._stream()))
        return out

    def score_small(self, v, rows, row_start, seed, step, mode, chain, want_F=False):
        """The same score for a small RBM in ONE launch (kurbm_score_small: csrc/kurbm_small.hip; at most 512 rows); returns a
        device tensor whose element 0 is the score (want_F: and a [2, rows] tensor of F(v), F(v'))."""
        with torch.cuda.device(self.device):
            ws = self.workspace(rows)
            opts = CdOpts(1, int(mode), 0.0, 0, None, None, int(seed), 0, int(step) & 0xFFFFFFFF, int(chain))
            out = self._alloc_floats(4, "score", zero=False)
            F = self._alloc_floats(2 * rows, "F", zero=False).view(2, rows) if want_F else None
            check(self.lib.kurbm_score_small(self.ctx.handle, C.byref(self.params), v.ptr(row_start), int(rows), v.ld, C.byref(opts),
                                             out.data_ptr(), F.data_ptr() if want_F else None, ws.data_ptr(), ws.numel(),
                                             self._stream()))
        return (out, F) if want_F else out

    def dump_plane(self, which, v, rows, mode=MODE_VISIBLE_BERNOULLI):
        """Test hook: one of the planes the last complete x3 CD-1 step on `rows` rows of v left in the workspace, as fp32
        [rows, units] (which: _lib.PLANE_*)."""
        with torch.cuda.device(self.device):
            vp = self._x3_pieces(v, None, mode)
            ws = self.workspace_bf16(rows, 1, 3, vp)
            units = self.n_vis if which in (_lib.PLANE_V_NEG, _lib.PLANE_V_NEG_T) else self.n_hid
            out = self._alloc_out(rows, units, "plane")
            check(self.lib.kurbm_x3_dump_plane(self.ctx.handle, int(which), int(rows), self.n_vis, self.n_hid, vp, int(mode),
                                               ws.data_ptr(), ws.numel(), out.ptr(), out.ld, self._stream()))
        return out

    def philox_uniform(self, rows, cols, seed, stream_id, step, row0=0):
        with torch.cuda.device(self.device):
            out = self._alloc_out(rows, cols, "uniform")
            rng = Rng(int(seed), int(row0), int(stream_id) & 0xFFFFFFFF, int(step) & 0xFFFFFFFF)
            check(self.lib.kurbm_philox_uniform(self.ctx.handle, out.ptr(), rows, cols, out.ld, C.byref(rng),
                                                self._stream()))
        return out

    def outer_delta(self, v_pos, h_pos, v_neg, h_neg, rows):
        """dW = v_pos^T.h_pos - v_neg^T.h_neg as a dense [n_vis, n_hid] tensor (test / bench hook)."""
        with torch.cuda.device(self.device):
            ws = self.workspace(rows)
            out = self._alloc_floats(self.n_vis * self.n_hid, "delta_w", zero=False).view(self.n_vis, self.n_hid)
            check(self.lib.kurbm_outer_delta(self.ctx.handle, v_pos.ptr(), h_pos.ptr(), v_neg.ptr(), h_neg.ptr(),
                                             rows, self.n_vis, self.n_hid, v_pos.ld, h_pos.ld, out.data_ptr(),
                                             ws.data_ptr(), ws.numel(), self._stream()))
        return out


def hidden_site(mode):
    """(activation, noise) of the v->h sampling site for an RBM mode (rbm.py:46-47 vs :58-59)."""
    return (ACT_RELU if mode == MODE_VISIBLE_GAUSSIAN else ACT_SIGMOID), NOISE_BERNOULLI


def visible_site(mode):
    """(activation, noise) of the h->v sampling site (rbm.py:52-53 vs :64-66)."""
    if mode == MODE_VISIBLE_GAUSSIAN:
        return ACT_LINEAR, NOISE_GAUSSIAN
    return ACT_SIGMOID, NOISE_BERNOULLI


__all__ = ["DeviceRBM", "DeviceMatrix", "ResidentPlanes", "resolve_device", "device_guard", "hidden_site", "visible_site", "round_up",
           "clamp_mask", "STREAM_GIBBS_H", "STREAM_GIBBS_V",
           "MODE_VISIBLE_BERNOULLI", "MODE_VISIBLE_GAUSSIAN", "MODE_COMPLEX", "NOISE_NONE"]
