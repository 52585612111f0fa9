"""CPU tier of the lattice tests (tests/lattice.py; the GPU tier is tests/test_gpu_lattice.py).

  * the certificate (S <= 2^22, float64 == fp32) and the coverage conditions hold for every fixture and shape the GPU tier uses;
  * emulate(), the fp32 restatement of the pieced product with its additions shuffled, equals float64 on all of them;
  * each fault emulate() can commit changes outputs of the fixture that targets it -- and, for the faults of the LOW piece, stays
    inside TOL = 1e-4 behind a sigmoid at synthetic_params weights: why the tolerance tiers cannot see them and this tier exists;
  * oracle.rbm_oracle's pre-activations equal the lattice reference exactly.
"""
import os
import sys

import numpy as np
import pytest

from oracle import rbm_oracle as O
from oracle.make_golden import synthetic_binary, synthetic_params

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lattice as L

TOL = 1e-4      # the bar of tests/test_gpu_parity.py on probabilities
BINARY = [("sparse", None), ("deep", None), ("dense", None)]
REAL = [("R1", None), ("R2", None), ("R3", None)]
ROUNDED = [("b8", None), ("b8", "b8n")]
ALL = BINARY + REAL + ROUNDED
IDS = ["%s%s" % (k, "" if d is None else "-" + d) for k, d in ALL]


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


@pytest.mark.parametrize("shape", list(L.SHAPES))
@pytest.mark.parametrize("kind,data_kind", ALL, ids=IDS)
def test_certificate_and_coverage(kind, data_kind, shape):
    p = L.Problem(kind, L.SHAPES[shape], data_kind=data_kind)
    for direction in ("vh", "hv"):
        fxs = p.fixtures(direction)
        for fx in fxs:
            assert L.certify(fx) <= L.S_MAX
            assert fx.ref().shape == (p.rows, p.n_hid if direction == "vh" else p.n_vis)
            if p.binary:
                assert np.isin(fx.ai, (0, 1)).all()
        L.coverage(fxs)
    W = p.params()[0]
    mid, lo = L.piece_shares(W)
    if kind == "sparse":
        assert mid == 1.0 and (np.count_nonzero(p.fixture("vh").ai, axis=1) <= 16).all()
    if kind in ("deep", "R3"):
        assert lo >= 0.9 and mid == 1.0
    if kind == "deep":
        assert (np.count_nonzero(p.fixture("vh").ai, axis=1) == 1).all() and np.abs(p.Wi).max() < (1 << 22) - 8191
    if kind == "dense":
        assert (p.fixture("vh").ai == 1).all() and np.abs(p.Wi).max() < 1 << 11
    if kind in ("R1", "b8"):
        assert (mid, lo) == (0.0, 0.0)                                   # one piece
    if kind == "R2":
        assert mid == 1.0 and lo == 0.0                                  # two pieces
    # the data operand's pieces
    a = p.fixture("vh").a
    amid = O.bf16_split3(a)[1][a != 0]
    alo = O.bf16_split3(a)[2][a != 0]
    if kind == "R1":
        assert (amid != 0).all() and (alo != 0).all()                    # three pieces
    if kind == "R2":
        assert (amid != 0).all() and (alo == 0).all()
    if kind == "R3":
        assert (amid == 0).all() and not np.isin(a[a != 0], (0.0, 1.0)).any()    # one bf16 piece that is no byte


def test_real_fixtures_exercise_all_six_kept_pairs_and_none_of_the_dropped():
    """Pairs (ia, ib) with non-zero pieces on both sides: R1 gives (0..2, 0), R2 (0..1, 0..1), R3 (0, 0..2) -- together the six
    pairs with ia + ib <= 2 -- and no fixture has a non-zero pair with ia + ib > 2, which the kernels leave out."""
    seen = set()
    for kind in ("R1", "R2", "R3"):
        p = L.Problem(kind, L.SHAPES["tiny"])
        fx = p.fixture("vh")
        na = [bool(np.any(x != 0)) for x in O.bf16_split3(fx.a)]
        nb = [bool(np.any(x != 0)) for x in O.bf16_split3(fx.b)]
        pairs = {(i, j) for i in range(3) for j in range(3) if na[i] and nb[j]}
        assert all(i + j <= 2 for i, j in pairs), (kind, pairs)
        seen |= pairs
    assert seen == {(i, j) for i in range(3) for j in range(3) if i + j <= 2}


@pytest.mark.parametrize("shape", list(L.SHAPES))
def test_statistics_and_update_fixtures(shape):
    for kind in ("binary", "six"):
        fx, planes = L.stats_problem(kind, L.SHAPES[shape])
        L.certify(fx)
        L.coverage([fx])
        vp, hp, vn, hn = (x.astype(np.float64) for x in planes)
        assert np.array_equal((vp.T @ hp - vn.T @ hn).astype(np.float32), fx.ref())
    for kind in ("sparse", "b8"):
        up = L.UpdateProblem(kind, L.SHAPES[shape])
        W, b_h, b_v = up.params()
        d = up.delta()
        nw = W.size
        for mom in (False, True):
            Wi, bhi, bvi, vw, _, _ = up.after(mom)
            vel = up.velocity()[0].astype(np.float64) * up.MU if mom else 0.0
            W1 = W.astype(np.float64) + vel + up.LR * d[:nw].reshape(W.shape).astype(np.float64)
            assert np.array_equal(W1, np.ldexp(Wi.astype(np.float64), up.eb))
            assert np.array_equal(W1.astype(np.float32).astype(np.float64), W1)
            if kind == "b8":
                assert np.array_equal(O.bf16_round(W1.astype(np.float32)), W1.astype(np.float32))      # the rounded mirror is exact
            for direction in ("vh", "hv"):
                fx = up.fixture(direction, mom)
                L.certify(fx)
                L.coverage([fx])
        assert np.mean(O.bf16_split3(up.fixture("vh", False).b)[2] != O.bf16_split3(W)[2]) > 0.5 or kind == "b8"


@pytest.mark.parametrize("shape", list(L.SHAPES))
@pytest.mark.parametrize("kind,data_kind", ALL, ids=IDS)
def test_emulation_without_a_fault_is_exact(kind, data_kind, shape):
    """fp32 accumulation of the piece products in a shuffled order, the byte plane's doubled operand halved at the end, equals the
    float64 result bit for bit: the certificate's claim, checked by doing it."""
    p = L.Problem(kind, L.SHAPES[shape], data_kind=data_kind)
    for direction in ("vh", "hv"):
        fx = p.fixture(direction)
        formats = (["bytes", 1, 3] if shape == "tiny" else ["bytes"]) if p.binary else [None]
        for fmt in formats:
            got = L.emulate(fx.a, fx.b, fx.bias, a_pieces=fmt, seed=5)
            assert np.array_equal(bits(got), bits(fx.ref())), (fx.name, fmt)


def test_each_fault_moves_the_lattice_and_hides_behind_the_tolerance():
    """What the tolerance tiers cannot see.  At synthetic_params weights (|W| <= 0.19), 0/1 data, 130 x 784 x 256, behind a
    sigmoid: a dropped low piece, a low piece lost in the last k element and a low piece left stale by an update all stay
    below TOL = 1e-4 (by more than a factor of ten), so a kernel variant that commits them passes every parity test.  On the
    lattice the same faults change the bits of most compared outputs.  Controls: middle and low piece lost together, and a
    whole k element left out, ARE seen by TOL (the last one only because synthetic data happens to be active there)."""
    B, nv, nh = 130, 784, 256
    W, b_h, _ = synthetic_params(nv, nh, seed=1)
    V = synthetic_binary(B, nv, seed=2, p=0.3)
    ref = O.sigmoid(V.astype(np.float64) @ W.astype(np.float64) + b_h.astype(np.float64))
    g = np.random.default_rng(3)
    W_old = (W - np.float32(1e-3) * g.standard_normal(W.shape).astype(np.float32)).astype(np.float32)
    moved = {}
    for fault, kw in (("none", {}), ("lo", dict(drop="lo")), ("lo@last_k", dict(drop="lo@last_k")),
                      ("stale_lo", dict(stale_lo_from=W_old)), ("mid+lo", dict(drop="mid+lo")), ("last_k", dict(drop="last_k"))):
        prob = O.sigmoid(L.emulate(V, W, b_h, **kw).astype(np.float64))
        moved[fault] = float(np.max(np.abs(prob - ref)))
    print("max |prob - float64| behind the sigmoid:", moved)
    assert moved["none"] <= 1e-6
    for fault in ("lo", "lo@last_k", "stale_lo"):
        assert moved[fault] <= TOL / 10, (fault, moved[fault])
    assert moved["mid+lo"] > TOL and moved["last_k"] > TOL

    shape = L.SHAPES["mid"]
    # a dropped piece: 'sparse' (every weight has a middle piece, most a low one) and 'deep' (one term per output)
    for kind, floor in (("sparse", 0.5), ("deep", 0.9)):
        fx = L.Problem(kind, shape).fixture("vh")
        got = L.emulate(fx.a, fx.b, fx.bias, drop="lo")
        share = float(np.mean(bits(got) != bits(fx.ref())))
        assert share >= floor, (kind, share)
    # the last k element: the rows of 'deep' whose single one sits there lose their low piece, and no other row changes
    p = L.Problem("deep", shape)
    hit = 0
    for fx in p.fixtures("vh"):
        rows_last = fx.ai[:, -1] != 0
        for drop in ("lo@last_k", "last_k"):
            wrong = (bits(L.emulate(fx.a, fx.b, fx.bias, drop=drop)) != bits(fx.ref())).any(axis=1)
            assert np.array_equal(wrong, rows_last), drop
        hit += int(rows_last.sum())
    assert hit >= 1                                     # (coverage: some call has a row there)
    # a stale low piece after an update
    up = L.UpdateProblem("sparse", shape)
    fx = up.fixture("vh", False)
    got = L.emulate(fx.a, fx.b, fx.bias, stale_lo_from=up.params()[0])
    assert np.mean(bits(got) != bits(fx.ref())) >= 0.5


@pytest.mark.parametrize("kind,data_kind", ALL, ids=IDS)
def test_oracle_preactivations_are_the_lattice_reference(kind, data_kind):
    """oracle.rbm_oracle computes a = v.W + b in fp32 (numpy's matmul, any order): on the lattice that is exact, so the oracle
    and the integer reference agree bit for bit -- relu(a) of the Gaussian mode's hidden site, the mean of its visible site."""
    p = L.Problem(kind, L.SHAPES["mid"], data_kind=data_kind)
    W, b_h, b_v = p.params()
    G = O.MODE_VISIBLE_GAUSSIAN
    fx = p.fixture("vh")
    assert np.array_equal(bits(O.hidden_prob(fx.a, W, b_h, G)), bits(fx.ref(relu=True)))
    fx = p.fixture("hv")
    loc = O.sample_visible(fx.a, W, b_v, O.Rng(1, 0), 7, G)[0]
    assert np.array_equal(bits(loc), bits(fx.ref()))


def test_census_of_the_x3_comparisons():
    """The numbers the tier's description quotes: (format, knob set, shape, direction) combinations of the x3 half steps and the
    outputs compared over them (no GPU work: the plan is walked on the host)."""
    from test_gpu_lattice import SHAPE_IDS, X3_KNOBS, x3_plan
    combos, outputs = set(), 0
    for shape in SHAPE_IDS:
        rows, nv, nh = L.SHAPES[shape]
        for ki, _ in enumerate(X3_KNOBS):
            for fmt, kind, direction, call, act, noise in x3_plan(shape):
                combos.add((fmt, ki, shape, direction))
                outputs += rows * (nh if direction == "vh" else nv)
    print("x3 half steps: %d (format, knob set, shape, direction) combinations, %d outputs compared" % (len(combos), outputs))
    assert len(combos) == 3 * len(X3_KNOBS) * 3 * 2
