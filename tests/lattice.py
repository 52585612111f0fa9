"""Lattice inputs for the linear GEMM hooks: operands on which exact arithmetic is the only right answer.

Every fixture here is a GEMM problem out = a @ b + bias whose operands are INTEGER multiples of power-of-two quanta (a: q_a,
b: q_b, bias: q_a * q_b) and small enough that every product and every partial sum, in any order and under any piece schedule,
is an integer multiple of q_a * q_b below 2^24 of it -- exactly an fp32 number.  The float64 result is then exactly an fp32
number too, and a kernel that accumulates in fp32 must return THOSE BITS whatever its tiling, split, block order or the order in
which it walks the bf16 pieces.  No tolerance is involved anywhere: tests/test_gpu_lattice.py compares uint32 views.

certify() is the proof obligation, in integer arithmetic: S = max over outputs of sum_k |a_k| |b_k| + |bias| <= 2^22 units.
fp32 holds 24 bits; the two spare bits pay for
  * the byte plane of 0/1 operands, whose "one" is the bf16 value 2.0 with the sum halved in the epilogue (partial sums are twice
    as large), and
  * bf16 pieces whose magnitudes overshoot: x = hi + mid + lo with round-to-nearest pieces of either sign, where
    |hi| + |mid| + |lo| <= (1 + 2^-7) |x|, so a partial sum of pieces can exceed the sum of the values it stands for.

When both operands are split into three pieces the kernels keep the six piece pairs with ia + ib <= 2 (pb_codes); a real-valued
fixture is exact only where the three dropped pairs vanish, which R1, R2 and R3 arrange by the number of significant bits.

Placement of the non-zero data is by stride and permutation, never by chance: every k index is active in some row by
construction (coverage() asserts it), so a fault at any k position reaches a compared output.

emulate() restates the pieced product in fp32 with the additions in a shuffled order, and can be told to commit the faults the
tier exists to catch (a dropped piece, a dropped last k element, a stale low piece after an update).
"""
import math

import numpy as np

from oracle import rbm_oracle as O

S_MAX = 1 << 22

# (rows, n_vis, n_hid): the smallest shapes that still reach each code path of the half-step kernels
SHAPES = {
    "tiny": (37, 70, 36),       # below one tile
    "mid": (200, 330, 137),     # an even number of 128-row tiles (256 x 64 tiling eligible), 6 and 3 k-tiles, a ragged column tile
    "wide": (500, 784, 260),    # 13 k-tiles (a half-filled 128-deep byte block), 4 row tiles, 3 column tiles
}


class Fixture:
    """out = a @ b + bias on the lattice.  ai [rows, K], bi [K, N], ci [N]: the integer numerators; ea, eb: log2 of the quanta."""

    def __init__(self, name, ai, ea, bi, eb, ci):
        self.name = name
        self.ai, self.bi, self.ci = (np.asarray(x, dtype=np.int64) for x in (ai, bi, ci))
        self.ea, self.eb = int(ea), int(eb)
        self.a = np.ldexp(self.ai.astype(np.float64), self.ea).astype(np.float32)
        self.b = np.ldexp(self.bi.astype(np.float64), self.eb).astype(np.float32)
        self.bias = np.ldexp(self.ci.astype(np.float64), self.ea + self.eb).astype(np.float32)
        # the numerators went into fp32 unchanged
        assert np.array_equal(np.ldexp(self.a.astype(np.float64), -self.ea), self.ai)
        assert np.array_equal(np.ldexp(self.b.astype(np.float64), -self.eb), self.bi)
        assert np.array_equal(np.ldexp(self.bias.astype(np.float64), -self.ea - self.eb), self.ci)

    def ref_int(self):
        return self.ai @ self.bi + self.ci

    def ref(self, relu=False):
        """The exact result as fp32 (certify() shows the cast changes nothing)."""
        r = np.ldexp(self.ref_int().astype(np.float64), self.ea + self.eb)
        if relu:
            r = np.maximum(r, 0.0)
        return r.astype(np.float32)


def certify(fx):
    """S <= 2^22 in integers, and the float64 product plus bias survives the round trip through fp32.  Returns S."""
    S = int((np.abs(fx.ai) @ np.abs(fx.bi) + np.abs(fx.ci)).max())
    assert S <= S_MAX, "%s: S = %d > 2^22" % (fx.name, S)
    r64 = fx.a.astype(np.float64) @ fx.b.astype(np.float64) + fx.bias.astype(np.float64)
    assert np.array_equal(np.ldexp(r64, -fx.ea - fx.eb), fx.ref_int()), fx.name      # float64 made no error
    assert np.array_equal(r64.astype(np.float32).astype(np.float64), r64), fx.name  # ... and fp32 holds it
    return S


def coverage(fxs):
    """Every k index is active in some row of the fixtures `fxs` (one problem, possibly several calls)."""
    active = np.zeros(fxs[0].ai.shape[1], bool)
    for fx in fxs:
        active |= (fx.ai != 0).any(axis=0)
    assert active.all(), "%s: k indices %s are never active" % (fxs[0].name, np.flatnonzero(~active)[:8])


def piece_shares(x):
    """(share of elements with a non-zero middle piece, ... a non-zero low piece) of the bf16 split the x3 path makes."""
    _, mid, lo = O.bf16_split3(np.ascontiguousarray(x, dtype=np.float32))
    return float(np.mean(mid != 0)), float(np.mean(lo != 0))


# ---- placement -------------------------------------------------------------------------------------------------------
def _stride(K):
    """A multiplier coprime to K near 0.38 K: consecutive slots land in different k-tiles."""
    g = max(1, int(0.381966 * K))
    while math.gcd(g, K) != 1:
        g += 1
    return g


def _slots(rows, K, per_row, call=0):
    """[rows, per_row] column indices: slot s = (call * rows + r) * per_row + j sits at column (s * g) mod K -- a permutation of
    a cyclic walk, so rows * per_row >= K consecutive slots touch every column."""
    per_row = min(per_row, K)
    s = (np.arange(rows)[:, None] + call * rows) * per_row + np.arange(per_row)[None, :]
    return (s * _stride(K)) % K


def _place(rows, K, per_row, values, call=0):
    """Integer data [rows, K]: values[r, j] at the slots of row r, zero elsewhere."""
    cols = _slots(rows, K, per_row, call)
    a = np.zeros((rows, K), np.int64)
    a[np.arange(rows)[:, None], cols] = values[:, : cols.shape[1]]
    assert (np.count_nonzero(a, axis=1) == cols.shape[1]).all()      # (per_row <= K distinct columns per row)
    return a


def calls_to_cover(rows, K, per_row):
    return -(-K // (rows * min(per_row, K)))


def _signs(g, shape):
    return 1 - 2 * g.integers(0, 2, shape)


def _three_piece(g, shape, top, low_bits):
    """Magnitudes A 2^(top-7) + B 2^(top-15) + C with A in [128, 256), B in [64, 128) and C < 2^low_bits no multiple of
    2^(low_bits - 1): hi = A ..., the middle piece is B ... rounded at 8 bits and the low piece is what is left -- non-zero BY
    CONSTRUCTION (an odd value alone does not force that: 2^21 + 1 is hi + mid).  top = position of A's leading bit."""
    assert top - 15 == low_bits + 0 and low_bits >= 2
    A = g.integers(128, 256, shape)
    B = g.integers(64, 128, shape)
    C = g.integers(1, 1 << low_bits, shape)
    half = 1 << (low_bits - 1)
    C = np.where(C % half == 0, C + 1, C)
    return (A << (top - 7)) + (B << (top - 15)) + C


def _odd(g, lo, hi, shape):
    return g.integers(lo // 2, hi // 2, shape) * 2 + 1


# ---- weights: integer numerators [K_vis, N_hid] ---------------------------------------------------------------------
def weights(kind, n_vis, n_hid, seed=0):
    """(numerators [n_vis, n_hid], log2 quantum) of the weight lattice of fixture `kind`."""
    g = np.random.default_rng(9000 + seed)
    sh = (n_vis, n_hid)
    if kind == "sparse":       # odd |m| in [2^16, 2^18): 17 or 18 significant bits, the middle piece never zero
        return _odd(g, 1 << 16, 1 << 18, sh) * _signs(g, sh), -16
    if kind == "deep":         # |m| < 2^22 - 2^13: three full pieces, the low one non-zero by construction
        return _three_piece(g, sh, 21, 6) * _signs(g, sh), -20
    if kind == "dense":        # |m| < 2^11
        return _odd(g, 1, 1 << 11, sh) * _signs(g, sh), -10
    if kind == "R1":           # <= 8 bits (here 3): one piece
        return g.integers(1, 8, sh) * _signs(g, sh), -3
    if kind == "R2":           # 10 bits, odd: two pieces
        return _odd(g, 1 << 9, 1 << 10, sh) * _signs(g, sh), -10
    if kind == "R3":           # 18 bits, three pieces, the low one non-zero by construction
        return _three_piece(g, sh, 17, 2) * _signs(g, sh), -17
    if kind == "b8":           # 8 bits: exactly bf16, so the rounded path is exact too
        return g.integers(128, 256, sh) * _signs(g, sh), -8
    raise ValueError(kind)


def bias(kind, n, seed=0):
    """Numerators of a bias vector [n] inside the bias budget of `kind` (units q_a q_b); every entry distinct from its
    neighbours, both signs."""
    budget = {"sparse": 15, "deep": 8191, "dense": (1 << 20) - 1, "R1": (1 << 18) - 1, "R2": 4095, "R3": (1 << 18) - 1,
              "b8": (1 << 19) - 1}[kind]
    j = np.arange(n, dtype=np.int64) + seed
    return ((j * 7919 + 13) % (2 * budget + 1)) - budget


# ---- data: integer numerators [rows, K] ------------------------------------------------------------------------------
def data(kind, rows, K, seed=0, call=0):
    """(numerators [rows, K], log2 quantum, is_binary) of the data operand of fixture `kind`."""
    g = np.random.default_rng(9500 + seed + 31 * call)
    if kind == "sparse":       # 0/1, at most 16 ones per row
        return _place(rows, K, 16, np.ones((rows, 16), np.int64), call), 0, True
    if kind == "deep":         # 0/1, ONE one per row: one term per output, nothing accumulates beyond the three pieces
        return _place(rows, K, 1, np.ones((rows, 1), np.int64), call), 0, True
    if kind == "dense":        # every entry 1
        return np.ones((rows, K), np.int64), 0, True
    if kind == "R1":           # 18 bits (three pieces, low piece non-zero), two actives per row
        return _place(rows, K, 2, _three_piece(g, (rows, 2), 17, 2) * _signs(g, (rows, 2)), call), -17, False
    if kind == "R2":           # 10 bits, odd (two pieces), four actives per row
        return _place(rows, K, 4, _odd(g, 1 << 9, 1 << 10, (rows, 4)) * _signs(g, (rows, 4)), call), -10, False
    if kind == "R3":           # 3 bits and never 0/1 (one bf16 piece that is no byte), two actives per row
        return _place(rows, K, 2, g.integers(2, 8, (rows, 2)) * _signs(g, (rows, 2)), call), 0, False
    if kind == "b8":           # 0/1 by a stride pattern, two thirds ones
        r, k = np.arange(rows)[:, None], np.arange(K)[None, :]
        return ((r + k) % 3 != 0).astype(np.int64), 0, True
    if kind == "b8n":          # 4-bit values 1 .. 15, dense: 4 + 8 + log2(784) < 22
        r, k = np.arange(rows)[:, None], np.arange(K)[None, :]
        return 1 + (r * 7 + k * 3) % 15, -4, False
    raise ValueError(kind)


PER_ROW = {"sparse": 16, "deep": 1, "R1": 2, "R2": 4, "R3": 2}


class Problem:
    """One RBM on the lattice: W [n_vis, n_hid] of `kind` with both biases, and the fixtures of both directions.
    vh(call): a = v [rows, n_vis], b = W, bias = b_h;  hv(call): a = h [rows, n_hid], b = W^T, bias = b_v.
    calls(direction): how many calls walk every k index (deep: rows < K needs several)."""

    def __init__(self, kind, shape, seed=0, data_kind=None):
        self.kind, self.data_kind, self.shape, self.seed = kind, data_kind or kind, shape, seed
        self.rows, self.n_vis, self.n_hid = shape
        self.Wi, self.eb = weights(kind, self.n_vis, self.n_hid, seed)
        self.bhi, self.bvi = bias(kind, self.n_hid, seed), bias(kind, self.n_vis, seed + 1)
        self.binary = data(self.data_kind, 1, 1)[2]
        self._cache = {}

    def calls(self, direction):
        K = self.n_vis if direction == "vh" else self.n_hid
        per = PER_ROW.get(self.data_kind)
        return 1 if per is None else calls_to_cover(self.rows, K, per)

    def fixture(self, direction, call=0, rows=None):
        key = (direction, call, rows)
        if key not in self._cache:
            rows_ = rows or self.rows
            vh = direction == "vh"
            ai, ea, _ = data(self.data_kind, rows_, self.n_vis if vh else self.n_hid, self.seed + (0 if vh else 7), call)
            self._cache[key] = Fixture("%s/%s %s call %d" % (self.kind, self.data_kind, direction, call), ai, ea,
                                       self.Wi if vh else self.Wi.T, self.eb, self.bhi if vh else self.bvi)
        return self._cache[key]

    def fixtures(self, direction):
        return [self.fixture(direction, c) for c in range(self.calls(direction))]

    def params(self):
        """(W, b_h, b_v) fp32.  The biases are in units of THEIR direction's q_a q_b; the data quantum is the same both ways."""
        return self.fixture("vh").b, self.fixture("vh").bias, self.fixture("hv").bias


# ---- the fp32 statistics GEMM: dW = v_pos^T h_pos - v_neg^T h_neg, k = the batch ------------------------------------------
def stats_problem(kind, shape, seed=0):
    """Four planes on the lattice and the product as ONE fixture: a = [v_pos^T | v_neg^T] (n_vis x 2 rows), b = [h_pos; -h_neg].
    kind 'binary': 0/1 visibles;  'six': visibles of <= 6 bits, a quarter of the rows active per unit.  Hiddens: 8 bits.
    S then covers sum |pos| + sum |neg| over the rows."""
    rows, nv, nh = shape
    g = np.random.default_rng(9900 + seed)
    r, k = np.arange(rows)[:, None], np.arange(nv)[None, :]
    if kind == "binary":
        vp, vn, ea = ((r + 2 * k) % 3 != 0).astype(np.int64), ((2 * r + k) % 5 < 2).astype(np.int64), 0
    else:
        vp = np.where((r + 3 * k) % 4 == 0, 1 + (r * 5 + k * 11) % 63, 0)
        vn = np.where((r + 3 * k) % 4 == 2, 1 + (r * 13 + k * 7) % 63, 0)
        ea = -6
    hp, hn = g.integers(0, 256, (rows, nh)), g.integers(0, 256, (rows, nh))
    fx = Fixture("stats-" + kind, np.concatenate([vp.T, vn.T], axis=1), ea, np.concatenate([hp, -hn], axis=0), -8, np.zeros(nh, np.int64))
    planes = tuple(np.ldexp(x.astype(np.float64), e).astype(np.float32) for x, e in ((vp, ea), (hp, -8), (vn, ea), (hn, -8)))
    return fx, planes


# ---- an update on the lattice ---------------------------------------------------------------------------------------
class UpdateProblem:
    """W' = W + lr * dW exactly: W = m 2^eb, the packed delta holds d 2^(eb + 3) and lr = 2^-3, so W' = (m + d) 2^eb, and with
    momentum mu = 0.5 on a velocity of EVEN numerators u: vel' = (u / 2 + d) 2^eb, W' = (m + u / 2 + d) 2^eb.  Magnitudes are
    chosen so that W' stays inside the weight range of `kind` ('sparse': |m'| < 2^18, three pieces; 'b8': |m'| < 2^8, exactly
    bf16) and the half steps on W' hold their certificate.  The biases move the same way in their own units."""
    LR, MU = 0.125, 0.5

    def __init__(self, kind, shape, seed=0):
        self.kind, self.shape = kind, shape
        rows, nv, nh = shape
        g = np.random.default_rng(9700 + seed)
        if kind == "sparse":
            m = _odd(g, 1 << 17, (1 << 17) + (1 << 16), (nv, nh)) * _signs(g, (nv, nh))      # 18 bits: a low piece to go stale
            dmax, self.eb, bmax = 1 << 14, -16, 3
        else:
            m = g.integers(64, 128, (nv, nh)) * _signs(g, (nv, nh))
            dmax, self.eb, bmax = 32, -8, 1 << 16
        self.m = m
        self.d = g.integers(-dmax + 1, dmax, (nv, nh))
        self.u = 2 * g.integers(-dmax + 1, dmax, (nv, nh))
        self.bh, self.bv = g.integers(-bmax, bmax + 1, nh), g.integers(-bmax, bmax + 1, nv)
        self.dbh, self.dbv = g.integers(-bmax, bmax + 1, nh), g.integers(-bmax, bmax + 1, nv)
        self.ubh, self.ubv = 2 * g.integers(-bmax, bmax + 1, nh), 2 * g.integers(-bmax, bmax + 1, nv)

    def _f(self, x, e=0):
        return np.ldexp(np.asarray(x, np.float64), self.eb + e).astype(np.float32)

    def params(self):
        return self._f(self.m), self._f(self.bh), self._f(self.bv)

    def delta(self):
        """The packed [dW | db_h | db_v] buffer: numerators d at quantum 2^(eb + 3)."""
        return np.concatenate([self._f(self.d, 3).reshape(-1), self._f(self.dbh, 3), self._f(self.dbv, 3)])

    def velocity(self):
        return self._f(self.u), self._f(self.ubh), self._f(self.ubv)

    def after(self, momentum):
        """Integer numerators (W', b_h', b_v', vel_W', vel_bh', vel_bv') of the exact update."""
        if momentum:
            vw, vh, vv = self.u // 2 + self.d, self.ubh // 2 + self.dbh, self.ubv // 2 + self.dbv
        else:
            vw, vh, vv = self.d, self.dbh, self.dbv
        return self.m + vw, self.bh + vh, self.bv + vv, vw, vh, vv

    def fixture(self, direction, momentum, updated=True):
        """The half-step fixture on the updated (or the original) weights, 'sparse' 0/1 data (b8: the stride pattern)."""
        rows, nv, nh = self.shape
        Wi, bhi, bvi = self.after(momentum)[:3] if updated else (self.m, self.bh, self.bv)
        vh = direction == "vh"
        ai, ea, _ = data(self.kind, rows, nv if vh else nh, 3)
        return Fixture("update-%s %s" % (self.kind, direction), ai, ea, Wi if vh else Wi.T, self.eb, bhi if vh else bvi)


# ---- the pieced product, restated in fp32 ---------------------------------------------------------------------------
def emulate(a, b, bias, drop=None, stale_lo_from=None, a_pieces=None, seed=0):
    """out = a @ b + bias as the x3 kernels form it, in fp32: b as its three bf16 pieces, a as a byte plane (0/1 data: the value
    2.0, the sum halved at the end), one bf16 piece or three (a_pieces 'bytes' / 1 / 3; None: by the values); the piece pairs
    with ia + ib <= 2; one fp32 addition per (pair, k) term IN A SHUFFLED ORDER; the bias last.
    Faults:  drop = 'lo' | 'mid+lo' (those pieces of b never multiplied), 'last_k' (the last k element left out altogether),
    'lo@last_k' (its low piece alone: a tail tile that loses it);  stale_lo_from = the weights BEFORE an update (their low
    piece multiplied instead of the new one: a mirror rewrite that left it stale)."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    K = a.shape[1]
    binary = bool(np.isin(a, (0.0, 1.0)).all())
    if a_pieces is None:
        a_pieces = "bytes" if binary else (1 if np.array_equal(O.bf16_round(a), a) else 3)
    if a_pieces == "bytes":
        assert binary
        pa, scale = [a * np.float32(2.0)], np.float32(0.5)
    else:
        pa, scale = (list(O.bf16_split3(a)) if a_pieces == 3 else [a]), np.float32(1.0)
        assert a_pieces == 3 or np.array_equal(O.bf16_round(a), a)
    pb = list(O.bf16_split3(b))
    if stale_lo_from is not None:
        pb[2] = O.bf16_split3(np.ascontiguousarray(stale_lo_from, np.float32))[2]
    dropped = {"lo": (2,), "mid+lo": (1, 2)}.get(drop, ())
    terms = [(ia, ib, k) for ia in range(len(pa)) for ib in range(3) for k in range(K)
             if ia + ib <= 2 and ib not in dropped and not (drop == "last_k" and k == K - 1)
             and not (drop == "lo@last_k" and k == K - 1 and ib == 2)]
    order = np.random.default_rng(seed).permutation(len(terms))
    nz_a = [np.any(p != 0, axis=0) for p in pa]
    nz_b = [np.any(p != 0, axis=1) for p in pb]
    acc = np.zeros((a.shape[0], b.shape[1]), np.float32)
    for t in order:
        ia, ib, k = terms[t]
        if nz_a[ia][k] and nz_b[ib][k]:
            acc += pa[ia][:, k, None] * pb[ib][None, k, :]        # (bf16 x bf16: the product is exact; the addition rounds)
    return acc * scale + np.asarray(bias, np.float32)[None, :]
