"""GPU: cmf_gemm against tests/gemm_ref.py (fp64, written from the header's contract and pinned on the CPU by
tests/test_gemm_ref_host.py), over the epilogue bodies, tile sizes, edge paths, prologues and split-K reductions of csrc/gemm.hip.

The kernel-against-kernel identities of the suite (persistent kernel, gathering GEMMs, fused BN-backward weight gradient: each
"bit-identical to cmf_gemm on the materialised tensor") are anchored to an independent reference through this module.

Every case owns its buffers: C is a column slice of a wider sentinel-filled buffer (padding and rows beyond M must stay
bit-unchanged), statistics and the split-K workspace start as NaN (every statistics slot must end finite), operands have padded
row strides.  Masks are fed grid-valued inputs (gemm_ref.grid: multiples of 1/4), so a * x + c is exact in fp32, both precisions
decide every element alike, nothing is excluded from a comparison, and exact zeros -- where `>` against `>=` and the slope at
zero show -- occur in every case (asserted).

Bounds: elements |C - ref| <= f * (tol * P + 1e-6), P = |A'| @ |B'|, f the epilogue's factor, tol = 2e-6 single pass / 4e-6
split-K (tests/test_gpu_gemm.py's _check); sigmoid rtol = atol = 2e-5.  Statistics of a partial over n rows: the propagated
element bounds + (n + 3) * 2^-24 * sum |term|.  Each check prints its worst err / bound ratio and reports it on failure.

Worst measured ratio per group on an MI355X (err / bound; 1.0 = at the bound; C = elements, s = statistics per 128-row slot,
S = statistics summed over the slots):
    forward (a)                C 0.279   s 0.046   S 0.031        accumulate               C 0.129
    forward, 256-row tile      C 0.191   s 0.042   S 0.004        (generic loop, per pair: 0.004)
    backward (b)               C 0.164   s 0.027   S 0.008        256-row tile             C 0.150   s 0.013
    persistent kernel          C 0.156   s 0.017   S 0.002
    weight gradient (c)        C 0.166 (single pass and every split_k; accumulate 0.165; staged interior loop 0.110)
    off-diagonal pairs (d)     C 0.161   s 0.031   S 0.007
The statistics ratios are small because their bound is dominated by the propagated element bounds.
"""

import pytest
import torch

from gemm_ref import elem_bound, gemm_ref, grid, stat_bound

pytestmark = pytest.mark.gpu

SENTINEL = -1234.5
NAN = float("nan")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture()
def L():
    """The library with its process-wide switches restored afterwards."""
    from cmflow_amd import _lib
    lib = _lib.lib()
    try:
        yield lib
    finally:
        lib.cmf_gemm_persist_config(1, 0)
        lib.cmf_thin_general(0)


def _r4(n):
    return (n + 3) // 4 * 4


def _p(t):
    return None if t is None else t.data_ptr()


def call_gemm(L, A, B, a_t, b_t, *, pro=None, prob=None, bias=None, act=0, stats=False, bwd=None, dxyz=None, split_k=1, prior=None,
              c_shift=4, ldc_odd=False, ldz_odd=False):
    """cmf_gemm through the C ABI on buffers built here from the logical A (M,K), B (K,N).  Returns (C, stats or None) after
    checking that nothing outside C's M x N block and the statistics slots was written."""
    from cmflow_amd import _lib
    dev = A.device
    (M, K), N = A.shape, B.shape[1]
    f32 = dict(dtype=torch.float32, device=dev)
    if a_t:
        Ab = torch.zeros(K, _r4(M) + 4, **f32); Ab[:, :M] = A.t()
    else:
        Ab = torch.zeros(M, _r4(K) + 4, **f32); Ab[:, :K] = A
    if b_t:
        Bb = torch.zeros(N, _r4(K) + 4, **f32); Bb[:, :K] = B.t()
    else:
        Bb = torch.zeros(K, _r4(N) + 8, **f32); Bb[:, :N] = B
    ldc = _r4(c_shift + N) + 8 + (1 if ldc_odd else 0)
    wide = torch.full((M + 2, ldc), SENTINEL, **f32)
    if prior is not None:
        wide[:M, c_shift:c_shift + N] = prior
    Cv = wide[:, c_shift:]
    st, nstat = None, 5 if (dxyz is not None and bwd is not None) else 2
    tiles = L.cmf_gemm_tiles_m(M)
    if stats:
        st = torch.full((tiles + 1, nstat, N), NAN, **f32)           # (+ one guard slot)
    ws = torch.full((split_k, M, N), NAN, **f32) if split_k > 1 else None
    mode, Zb, ldz, ea, ec, em, ei = 0, None, 0, None, None, None, None
    if bwd is not None:
        mode = bwd[0]
        ldz = _r4(N) + 8 + (1 if ldz_odd else 0)
        Zb = torch.zeros(M, ldz, **f32); Zb[:, :N] = bwd[1]
        if mode == 1:
            ea, ec, em, ei = (t.contiguous() for t in bwd[2:6])
    d4 = dxyz.contiguous() if (dxyz is not None and bwd is not None) else None
    err = L.cmf_gemm(M, N, K, int(a_t), int(b_t), Ab.data_ptr(), Ab.stride(0), Bb.data_ptr(), Bb.stride(0), Cv.data_ptr(), ldc,
                     _p(pro[0]) if pro else None, _p(pro[1]) if pro else None, _p(prob[0]) if prob else None,
                     _p(prob[1]) if prob else None, _p(bias), act, _p(st), mode, _p(Zb), ldz, _p(ea), _p(ec), _p(em), _p(ei), _p(d4),
                     split_k, _p(ws), int(prior is not None), _lib.stream_ptr())
    _lib.check(err, "cmf_gemm")
    torch.cuda.synchronize()
    C = wide[:M, c_shift:c_shift + N].clone()
    wide[:M, c_shift:c_shift + N] = SENTINEL
    assert bool((wide == SENTINEL).all()), "cmf_gemm wrote outside the M x N block of C"
    if stats:
        assert bool(torch.isnan(st[tiles]).all()), "cmf_gemm wrote past its statistics slots"
        assert bool(torch.isfinite(st[:tiles]).all()), "a statistics slot was left unwritten or is not finite"
        st = st[:tiles]
    return C, st


def _ratio(err, bound):
    return float((err / bound.clamp_min(1e-300)).masked_fill((err == 0) & (bound == 0), 0.0).max())


def judge(name, C, st, ref, tol, per_slot=True, slot_rows=128):
    """Elements and statistics against the reference; prints the worst ratios, fails above 1."""
    worst = {"C": _ratio((C.double() - ref.C).abs(), elem_bound(ref, tol))}
    if st is not None:
        M, N = ref.C.shape
        tiles = st.shape[0]
        pad = torch.zeros(tiles * 128 - M, N, dtype=torch.float64, device=C.device) if tiles * 128 > M else None

        def slots(t):
            return (torch.cat((t, pad)) if pad is not None else t[:tiles * 128]).view(tiles, 128, N).sum(1)
        for which, term in enumerate(ref.terms):
            if term is None:
                continue                                             # unspecified row: finite (checked by call_gemm)
            got = st[:, which].double()
            want, bound = slots(term), slots(stat_bound(ref, which, tol, slot_rows))
            if per_slot:
                worst["s%d" % which] = _ratio((got - want).abs(), bound)
            worst["S%d" % which] = _ratio((got.sum(0) - want.sum(0)).abs(), bound.sum(0))
    print("RATIO %s %s" % (name, " ".join("%s=%.3f" % kv for kv in sorted(worst.items()))))
    bad = {k: v for k, v in worst.items() if not v <= 1.0}
    assert not bad, (name, bad)


def _gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)) % (2 ** 31))


# ---- (a) forward layout (A[M][K], W[N][K]), epilogue kind 1 -------------------------------------------------------------------

FWD_OPTS = [(True, True, 1, True), (True, False, 0, True), (False, True, 2, False), (True, True, 3, True)]
FWD_SHAPES = [
    (64, 64, 48), (50, 40, 24),                                      # 64 x 64: fast_epilogue / generic edge
    (64, 256, 48), (33, 130, 20),                                    # 64 x 128
    (256, 64, 48), (300, 60, 100),                                   # 128 x 64 direct_epilogue; edge + ragged contraction
    (384, 256, 64), (1000, 192, 100), (130, 132, 1028),              # 128 x 128 direct_epilogue + edge tiles both ways, ragged K
    (300, 3, 64), (300, 3, 48), (257, 77, 36),                       # N % 4 != 0: scalar stores (thin kernel; tiled; tiled)
    (128 * 7 - 5, 128, 32), (128 * 8 - 5, 128, 32), (128 * 9 - 5, 128, 32), (128 * 17 - 5, 128, 32),   # row panels over 8 XCDs
]
# accumulate onto a prior: one interior and one edge shape per tile size
ACC_SHAPES = [(64, 64, 48), (50, 40, 24), (64, 256, 48), (33, 130, 20), (256, 64, 48), (300, 60, 100), (384, 256, 64), (1000, 192, 100)]


def _fwd_inputs(dev, M, N, K, pro, bias):
    g = _gen(M, N, K, pro, bias)
    A = (grid((M, K), -2, 2, g) if pro else torch.randn(M, K, generator=g)).to(dev)
    W = torch.randn(N, K, generator=g).to(dev)
    pr = (grid((K,), 0.5, 2, g).to(dev), grid((K,), -2, 2, g).to(dev)) if pro else None
    b = torch.randn(N, generator=g).to(dev) if bias else None
    return A, W, pr, b


@pytest.mark.parametrize("pro,bias,act,stats", FWD_OPTS)
@pytest.mark.parametrize("M,N,K", FWD_SHAPES)
def test_forward_epilogues(dev, L, M, N, K, pro, bias, act, stats):
    A, W, pr, b = _fwd_inputs(dev, M, N, K, pro, bias)
    if pro:
        assert bool((pr[1] > 0).any())                               # a zero-filled k must give 0, not relu(pro_c[k]) * W
    C, st = call_gemm(L, A, W.t(), False, True, pro=pr, bias=b, act=act, stats=stats)
    judge("fwd", C, st, gemm_ref(A, W.t(), pro=pr, bias=b, act=act), 2e-6)


@pytest.mark.parametrize("M,N,K", ACC_SHAPES)
def test_forward_accumulate(dev, L, M, N, K):
    A, W, pr, b = _fwd_inputs(dev, M, N, K, True, True)
    prior = torch.randn(M, N, generator=_gen(M, N)).to(dev)
    C, _ = call_gemm(L, A, W.t(), False, True, pro=pr, bias=b, act=1, prior=prior)
    judge("fwd_acc", C, None, gemm_ref(A, W.t(), pro=pr, bias=b, act=1, prior=prior), 2e-6)


@pytest.mark.parametrize("pro,bias,act", [(True, True, 1), (False, False, 0), (True, True, 3)])
def test_forward_256_row_tile(dev, L, pro, bias, act):
    """(24576, 512, 32): the 256 x 128 tile.  Its direct_epilogue (the first two cases) gives each 128-row half its own partial;
    the generic loop (sigmoid) writes the tile's sums into the first of its two slots and exact zeros into the second.  Both
    are judged per slot pair against fp64, and the form each body documents is asserted."""
    M, N, K = 24576, 512, 32
    A, W, pr, b = _fwd_inputs(dev, M, N, K, pro, bias)
    C, st = call_gemm(L, A, W.t(), False, True, pro=pr, bias=b, act=act, stats=True)
    ref = gemm_ref(A, W.t(), pro=pr, bias=b, act=act)
    pair = st.view(M // 256, 2, 2, N)
    judge("fwd256", C, st, ref, 2e-6, per_slot=(act != 3), slot_rows=256 if act == 3 else 128)
    if act == 3:
        assert bool((pair[:, 1] == 0.0).all()), "second statistics slot of a 256-row tile (generic loop) must be exactly 0"
        for w in (0, 1):
            want = ref.terms[w].view(M // 256, 256, N).sum(1)
            bound = stat_bound(ref, w, 2e-6, 256).view(M // 256, 256, N).sum(1)
            r = _ratio((pair[:, 0, w].double() - want).abs(), bound)
            print("RATIO fwd256_pair s%d=%.3f" % (w, r))
            assert r <= 1.0, r


# ---- (b) data gradient (dZ[M][K], W[K][N]), kinds 2-5 -------------------------------------------------------------------------

BWD_OPTS = [(1, False, True), (1, True, True), (2, False, False), (2, True, True), (3, False, False), (3, True, True), (3, False, True)]
BWD_SHAPES = [
    (64, 64, 48, ""), (64, 128, 32, ""), (256, 64, 48, ""),          # fast_epilogue: 64-row tiles, 64-column tiles
    (256, 128, 32, ""), (1152, 256, 64, ""), (2048, 128, 256, ""),   # wave_epilogue (persistence off)
    (1000, 192, 96, ""), (130, 100, 40, ""),                         # generic loop: edges
    (256, 128, 32, "ldz"), (256, 128, 32, "ldc"),                    # generic loop: vector path off on an interior shape
]


def _bwd_inputs(dev, M, N, K, mode, dxyz):
    g = _gen(M, N, K, mode, dxyz)
    dZ = torch.randn(M, K, generator=g).to(dev)
    W = torch.randn(K, N, generator=g).to(dev)
    Z = grid((M, N), -2, 2, g).to(dev)
    ea, ec = grid((N,), 0.5, 2, g).to(dev), grid((N,), -2, 2, g).to(dev)
    mean, invstd = torch.randn(N, generator=g).to(dev), (torch.rand(N, generator=g) + 0.5).to(dev)
    d4 = torch.randn(M, 4, generator=g)
    d4[:, 3] = 0
    bwd = (1, Z, ea, ec, mean, invstd) if mode == 1 else (mode, Z)
    zero = (ea.double() * Z.double() + ec.double()) == 0 if mode == 1 else Z == 0
    assert bool(zero.any()), "the case must contain an exact zero at the mask"
    return dZ, W, bwd, (d4.to(dev) if dxyz else None)


def _bwd_case(dev, L, name, M, N, K, mode, dxyz, stats, variant="", **judge_kw):
    dZ, W, bwd, d4 = _bwd_inputs(dev, M, N, K, mode, dxyz)
    C, st = call_gemm(L, dZ, W, False, False, bwd=bwd, dxyz=d4, stats=stats, ldz_odd=variant == "ldz", ldc_odd=variant == "ldc")
    judge(name, C, st, gemm_ref(dZ, W, bwd=bwd, dxyz=d4), 2e-6, **judge_kw)


@pytest.mark.parametrize("mode,dxyz,stats", BWD_OPTS)
@pytest.mark.parametrize("M,N,K,variant", BWD_SHAPES)
def test_backward_epilogues(dev, L, M, N, K, variant, mode, dxyz, stats):
    assert L.cmf_gemm_persist_config(0, 0) == 0
    _bwd_case(dev, L, "bwd", M, N, K, mode, dxyz, stats, variant)


def test_backward_256_row_tile(dev, L):
    assert L.cmf_gemm_persist_config(0, 0) == 0
    _bwd_case(dev, L, "bwd256", 24576, 512, 32, 1, True, True)


@pytest.mark.parametrize("M,N,K", [(1024, 256, 192), (2048, 128, 256)])
@pytest.mark.parametrize("mode,dxyz,stats", [(1, True, True), (2, False, False)])
def test_persistent_kernel_against_fp64(dev, L, M, N, K, mode, dxyz, stats):
    assert L.cmf_gemm_persist_config(2, 8) == 0
    _bwd_case(dev, L, "persist", M, N, K, mode, dxyz, stats)


# ---- (c) weight-gradient layouts (A[K][M]; B[K][N] or B[N][K]): single pass and split-K ------------------------------------------

SPLITS = (1, 3, 8, 11, 16, 64, 96)


def _dw_inputs(dev, rows, cout, cin, prob):
    g = _gen(rows, cout, cin, prob)
    dZ = torch.randn(rows, cout, generator=g).to(dev)
    X = (grid((rows, cin), -2, 2, g) if prob else torch.randn(rows, cin, generator=g)).to(dev)
    q = (grid((cin,), 0.5, 2, g).to(dev), grid((cin,), -2, 2, g).to(dev)) if prob else None
    if prob:
        assert bool((q[1] > 0).any())
    return dZ, X, q


@pytest.mark.parametrize("rows", [2048, 1000, 40])
@pytest.mark.parametrize("cout,cin", [(128, 128), (256, 192), (130, 100), (40, 72), (40, 70)])
@pytest.mark.parametrize("b_t,prob", [(False, False), (False, True), (True, False)])
def test_weight_gradient_split_k(dev, L, rows, cout, cin, b_t, prob):
    """Slab counts that are no multiple of 8, slabs left empty (40 rows = 3 chunks), the wide reduction (128 x 128 with 64 / 96
    slabs), the scalar reduction (cin = 70), accumulate through each, and run-to-run bit identity.  One reference per case."""
    dZ, X, q = _dw_inputs(dev, rows, cout, cin, prob)
    ref = gemm_ref(dZ.t(), X, prob=q)
    prior = torch.randn(cout, cin, generator=_gen(cout, cin)).to(dev)
    ref_acc = gemm_ref(dZ.t(), X, prob=q, prior=prior)
    for split in SPLITS:
        tol = 2e-6 if split == 1 else 4e-6
        C, _ = call_gemm(L, dZ.t(), X, True, b_t, prob=q, split_k=split)
        judge("dw split=%d" % split, C, None, ref, tol)
        C2, _ = call_gemm(L, dZ.t(), X, True, b_t, prob=q, split_k=split)
        assert torch.equal(C, C2), "two calls at split_k = %d differ" % split
        if split in (1, 11, 96):                                     # single pass; float4 / scalar reduction; wide reduction at 128 x 128
            Ca, _ = call_gemm(L, dZ.t(), X, True, b_t, prob=q, split_k=split, prior=prior)
            judge("dw acc split=%d" % split, Ca, None, ref_acc, tol)


@pytest.mark.parametrize("split", [1, 16])
def test_weight_gradient_staged_interior_loop(dev, L, split):
    """32768 rows with the B prologue at 128 x 128: the register-staged interior loop (staged_dw)."""
    dZ, X, q = _dw_inputs(dev, 32768, 128, 128, True)
    C, _ = call_gemm(L, dZ.t(), X, True, False, prob=q, split_k=split)
    judge("dw staged split=%d" % split, C, None, gemm_ref(dZ.t(), X, prob=q), 2e-6 if split == 1 else 4e-6)


# ---- (d) (layout, kind) pairs without an instantiated fast path: the kind-0 kernel's generic loop -------------------------------

@pytest.mark.parametrize("M,N,K", [(256, 128, 48), (130, 100, 40)])
@pytest.mark.parametrize("pair", ["bias_act_nn", "stats_tt", "bias_tn"])
def test_off_diagonal_layout_kind_pairs(dev, L, M, N, K, pair):
    g = _gen(M, N, K, len(pair))
    A, B, b = torch.randn(M, K, generator=g).to(dev), torch.randn(K, N, generator=g).to(dev), torch.randn(N, generator=g).to(dev)
    if pair == "bias_act_nn":
        C, st = call_gemm(L, A, B, False, False, bias=b, act=2)
        ref = gemm_ref(A, B, bias=b, act=2)
    elif pair == "stats_tt":
        C, st = call_gemm(L, A, B, True, True, stats=True)
        ref = gemm_ref(A, B)
    else:
        C, st = call_gemm(L, A, B, True, False, bias=b)
        ref = gemm_ref(A, B, bias=b)
    judge(pair, C, st, ref, 2e-6)


# ---- (e) non-finite operands reach the output --------------------------------------------------------------------------------

@pytest.mark.parametrize("bad", [NAN, float("inf")])
@pytest.mark.parametrize("M,N,K,a_t,b_t,which,pos", [
    (130, 128, 32, False, True, "A", (5, 8)),                        # A[M][K], k % 4 == 0, on an M-edge tile
    (130, 128, 32, False, True, "A", (129, 0)),                      # ... in the edge tile's last valid row
    (130, 100, 40, False, False, "B", (8, 4)),                       # B[K][N], n % 4 == 0, edge shape
    (128, 128, 40, False, False, "B", (36, 64)),                     # interior shape, ragged K
    (128, 128, 40, True, False, "B", (3, 0)),
])
def test_non_finite_operand_reaches_its_row_or_column(dev, L, M, N, K, a_t, b_t, which, pos, bad):
    """Plain epilogue, no prologue: one NaN / +inf in a valid operand element makes exactly its row (A) or column (B) of C
    non-finite.  (The register-staged loads once marked out-of-range rows by a NaN in the data and swallowed these.)"""
    g = _gen(M, N, K, pos[0], pos[1])
    A, B = torch.randn(M, K, generator=g).to(dev), torch.randn(K, N, generator=g).to(dev)
    (A if which == "A" else B)[pos] = bad
    assert L.cmf_gemm_persist_config(0, 0) == 0
    C, _ = call_gemm(L, A, B, a_t, b_t)
    want = torch.zeros(M, N, dtype=torch.bool, device=dev)
    if which == "A":
        want[pos[0], :] = True
    else:
        want[:, pos[1]] = True
    assert torch.equal(~torch.isfinite(C), want), (int((~torch.isfinite(C)).sum()), int(want.sum()))
    fin = gemm_ref(torch.nan_to_num(A, 0.0, 0.0, 0.0), torch.nan_to_num(B, 0.0, 0.0, 0.0))
    err = torch.where(want, torch.zeros_like(fin.C), (C.double() - fin.C).abs())
    assert _ratio(err, elem_bound(fin, 2e-6)) <= 1.0


@pytest.mark.parametrize("bad", [NAN, float("inf")])
def test_non_finite_operand_in_the_staged_weight_gradient(dev, L, bad):
    """The staged_dw loop is reached only with the B prologue, B' = relu(prob_a * B + prob_c), which the kernels form with fmaxf:
    +inf stays +inf and makes column n of C non-finite; a NaN becomes 0 under fmaxf on every path, so for it the contract fixed
    here is that it disturbs NOTHING ELSE -- the other three columns of its float4 keep their values."""
    rows, cout, cin, k, n = 32768, 128, 128, 20001, 64
    dZ, X, q = _dw_inputs(dev, rows, cout, cin, True)
    X[k, n] = bad
    C, _ = call_gemm(L, dZ.t(), X, True, False, prob=q)
    Xf = X.clone()
    Xf[k, n] = 0.0
    ref = gemm_ref(dZ.t(), Xf, prob=q)
    other = torch.ones(cin, dtype=torch.bool, device=dev)
    other[n] = False
    assert bool(torch.isfinite(C[:, other]).all())
    assert _ratio((C.double() - ref.C).abs()[:, other], elem_bound(ref, 2e-6)[:, other]) <= 1.0
    if bad == float("inf"):
        assert bool((~torch.isfinite(C[:, n])).all())
