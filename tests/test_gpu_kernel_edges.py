"""Exact-arithmetic and launch-edge parity tests for the HIP kernels.

Inputs are small integers or dyadic values (tests/kernel_edges.py), so
every reduction is exact in fp32 in any order and the kernel must equal
the fp64 reference BITWISE. Tolerances remain only behind expf / log1pf /
sqrtf (loss 1e-5, dO 1e-7 at inv_b = 1/500, Adam 1e-6 / 1e-7 / 1e-7),
measured against fp64. Shapes are the smallest that take the unrolled
loops, every template instantiation and, for the launches with a grid cap
of their own (cbow_fwd_scalar and the eval kernels at 2048 blocks or their
env knob, the fused adam_rank1 at 1024, gemv_rows at 8192, gemv_cols at
2048), the second grid-stride iteration. The launches sized by grid_for
alone (walks, pcc_edges, cbow_fwd, trunc_normal, bf16_copy, adam_dense)
start a second sweep only past 2^20 blocks: test_gpu_scale.py covers
that. All tests need an MI355X (marked gpu); the CPU twins that validate
these inputs live in test_kernel_edges_cpu.py."""
import pytest
import torch

import kernel_edges as ke
from g2vec_amd import ops

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _dev(*ts):
    return tuple(t.to(DEV) for t in ts)


def _max_err(got, ref64):
    return float((got.detach().cpu().double() - ref64).abs().max())


# ================================================================ walks
def _gpu_walks(name):
    rp, ci, w, src, rep, L, seed, oracle = ke.walk_case(name)
    got = ops.random_walks(*_dev(rp, ci, w, src), rep, L, seed)
    return got, oracle, rp


def test_walks_bitwise_nonuniform_weights():
    """Integer weights 0..8 on a graph mixing the lean (<= 64), register
    (65..256) and chunked (> 256) sampling paths, rows anywhere in the CSR,
    a degree-0 source, an all-zero-weight row, len_path 100 (strided
    output loop): nodes, lengths and hashes equal the oracle's."""
    (gn, gl, gh), (on, ol, oh), rp = _gpu_walks("mixed")
    lean, reg, chunked = ke.steps_per_sampling_path(rp, on)
    assert min(lean, reg, chunked) >= 1000, (lean, reg, chunked)
    assert torch.equal(gl.cpu(), ol)
    assert torch.equal(gn.cpu(), on)
    assert torch.equal(gh.cpu(), oh)


@pytest.mark.parametrize("name,longer_than", [("len200", 128),
                                              ("len512", 256)])
def test_walks_len_path_edges(name, longer_than):
    """len_path 200 (hash table 512 slots) and 512 (the maximum, 1024
    slots) on a graph dense enough that walks outgrow 128 / 256 nodes."""
    (gn, gl, gh), (on, ol, oh), _ = _gpu_walks(name)
    assert int(ol.max()) > longer_than
    assert torch.equal(gl.cpu(), ol)
    assert torch.equal(gn.cpu(), on)
    assert torch.equal(gh.cpu(), oh)


@pytest.mark.parametrize("len_path", [0, 513])
def test_walks_len_path_out_of_range_raises(len_path):
    rp, ci, w, src, rep, _, seed, _ = ke.walk_case("len200")
    with pytest.raises(RuntimeError, match="len_path"):
        ops.random_walks(*_dev(rp, ci, w, src), rep, len_path, seed)


def test_walks_shard_invariance():
    """A permuted subset of the sources (every third node, reversed) gives,
    row for row, the full run's walk of the same (source, repetition)."""
    rp, ci, w, src, rep, L, seed, _ = ke.walk_case("mixed")
    d = _dev(rp, ci, w)
    fn, fl, fh = ops.random_walks(*d, src.to(DEV), rep, L, seed)
    sub = torch.flip(src[::3], dims=[0]).contiguous()
    sn, sl, sh = ops.random_walks(*d, sub.to(DEV), rep, L, seed)
    n_full, n_sub = len(src), len(sub)
    rows = torch.cat([r * n_full + sub.long() for r in range(rep)]).to(DEV)
    assert sn.shape[0] == rep * n_sub
    assert torch.equal(sn, fn[rows])
    assert torch.equal(sl, fl[rows])
    assert torch.equal(sh, fh[rows])


def test_walks_first_step_distribution_per_path():
    """Real-valued weights, one source row per sampling path (degree 40,
    200, 300, none at CSR offset 0): first-step counts follow w / sum(w)
    (chi-square below its 1e-6 upper quantile) and zero-weight neighbours
    are never chosen."""
    rp, ci, w = ke.distribution_graph()
    src = torch.tensor(ke.DIST_SOURCES, dtype=torch.int32)
    nodes, lengths, _ = ops.random_walks(*_dev(rp, ci, w, src), ke.DIST_REPS,
                                         2, ke.DIST_SEED)
    assert int(lengths.min()) == 2 and int(lengths.max()) == 2
    for chi2, df, zero_hits, off_row in ke.first_step_chi2(rp, ci, w,
                                                           nodes.cpu()):
        limit = ke.chi2_upper_quantile(df)
        print("chi2", chi2, "df", df, "limit", limit)
        assert zero_hits == 0 and off_row == 0
        assert chi2 < limit


# ============================================= scalar CBOW fwd and evals
def _s_table(seed=3, zero=False):
    if zero:
        return torch.zeros(ke.CBOW_G)
    return ke.dyadic(torch.Generator().manual_seed(seed), (ke.CBOW_G,), 8)


def _check_scalar_fwd(s, genes, offs, labels, inv_b):
    o, loss, correct, dO = ke.cbow_scalar_ref64(s, genes, offs, labels, inv_b)
    lg, cg, dg = ops.cbow_fwd_scalar(*_dev(s, genes, offs, labels), inv_b,
                                     True)
    print("loss err", _max_err(lg, loss), "dO err", _max_err(dg, dO))
    assert ke.bitwise_equal(cg, correct)
    assert _max_err(lg, loss) <= 1e-5
    assert _max_err(dg, dO) <= ke.dO_tol(inv_b)
    return o


@pytest.mark.parametrize("zero_s", [False, True])
def test_cbow_fwd_scalar_exact_inputs(zero_s):
    """Path lengths 1/15/16/17/31/32/33/~80 around the 16-lane sub-wave;
    dyadic s makes o exact, so `correct` must equal the oracle's on every
    path. s = 0 is the o == 0 tie: predicted class 0."""
    genes, offs, labels = ke.cbow_pathset()
    o = _check_scalar_fwd(_s_table(zero=zero_s), genes, offs, labels, 1 / 500)
    if zero_s:
        assert float(o.abs().max()) == 0.0
    else:
        assert int((o == 0).sum()) > 0        # natural ties are present too


def test_cbow_fwd_scalar_grid_stride():
    """P = 40000 > 2048 blocks x 16 paths: the grid-stride loop runs a
    second time."""
    genes, offs, labels = ke.cbow_pathset(P=40000, short=True)
    _check_scalar_fwd(_s_table(), genes, offs, labels, 1 / 40000)


def _eval_counts(s, genes, offs, labels, p_split, inv_b, P, scan=False,
                 sentinel=-7.0):
    counts = torch.zeros(2, device=DEV)
    dO = torch.full((P,), sentinel, device=DEV)
    sc = None
    if scan:
        lens = (offs[1:] - offs[:-1]).long()
        pathid = torch.repeat_interleave(
            torch.arange(P, dtype=torch.int32), lens).to(DEV)
        cap = int(lens.max()) // 64 + 2
        sc = (pathid, torch.empty(P * cap, device=DEV), cap)
    ops.cbow_eval_counts_(*_dev(s, genes, offs, labels), p_split, counts,
                          dO=dO, inv_b=inv_b, scan=sc)
    return counts.cpu(), dO.cpu()


def _check_eval(counts, dO, ref, p_split, inv_b, sentinel=-7.0):
    _o, _loss, correct, dref = ref
    assert float(counts[0]) == float(correct[:p_split].sum())
    assert float(counts[1]) == float(correct[p_split:].sum())
    if p_split:
        print("dO err", _max_err(dO[:p_split], dref[:p_split]))
        assert _max_err(dO[:p_split], dref[:p_split]) <= ke.dO_tol(inv_b)
    assert bool((dO[p_split:] == sentinel).all())     # untouched


def test_cbow_eval_counts_grid_stride_and_lds_bitwise(monkeypatch):
    """Grid caps of 2 blocks (G2VEC_EVAL_GRID / G2VEC_EVAL_LDS_GRID) at
    P = 2003: every sub-wave strides ~60 times. Counts equal the oracle's
    exactly, and the LDS variant is bitwise equal to the default."""
    genes, offs, labels = ke.cbow_pathset()
    P = labels.numel()
    s, p_split, inv_b = _s_table(), 1500, 1 / 1500
    ref = ke.cbow_scalar_ref64(s, genes, offs, labels, inv_b)
    monkeypatch.delenv("G2VEC_EVAL_LDS", raising=False)
    monkeypatch.setenv("G2VEC_EVAL_GRID", "2")
    ca, da = _eval_counts(s, genes, offs, labels, p_split, inv_b, P)
    _check_eval(ca, da, ref, p_split, inv_b)
    monkeypatch.setenv("G2VEC_EVAL_LDS", str(64 * 1024))
    monkeypatch.setenv("G2VEC_EVAL_LDS_GRID", "2")
    cb, db = _eval_counts(s, genes, offs, labels, p_split, inv_b, P)
    _check_eval(cb, db, ref, p_split, inv_b)
    assert torch.equal(ca, cb) and torch.equal(da, db)
    # and the uncapped default launch computes the same thing
    monkeypatch.delenv("G2VEC_EVAL_LDS")
    monkeypatch.delenv("G2VEC_EVAL_GRID")
    cc, dc = _eval_counts(s, genes, offs, labels, p_split, inv_b, P)
    assert torch.equal(ca, cc) and torch.equal(da, dc)


@pytest.mark.parametrize("p_split", [0, 1, 1003, 2002, 2003])
@pytest.mark.parametrize("variant", ["subwave", "lds", "scan"])
def test_cbow_eval_split_edges(monkeypatch, variant, p_split):
    """p_split at 0, 1, P-1, P and a non-multiple of 16: counts are exact
    and dO entries at and beyond p_split keep their sentinel."""
    genes, offs, labels = ke.cbow_pathset()
    P = labels.numel()
    assert P == 2003
    s, inv_b = _s_table(), 1 / 500
    ref = ke.cbow_scalar_ref64(s, genes, offs, labels, inv_b)
    monkeypatch.delenv("G2VEC_EVAL_GRID", raising=False)
    monkeypatch.delenv("G2VEC_EVAL_LDS", raising=False)
    if variant == "lds":
        monkeypatch.setenv("G2VEC_EVAL_LDS", str(64 * 1024))
    c, d = _eval_counts(s, genes, offs, labels, p_split, inv_b, P,
                        scan=(variant == "scan"))
    _check_eval(c, d, ref, p_split, inv_b)


@pytest.mark.parametrize("zero_s", [False, True])
def test_cbow_eval_scan_bitwise_equals_subwave(monkeypatch, zero_s):
    """With exact s the segmented-scan eval and the sub-wave eval see the
    same o on every path: equal counts, bitwise equal dO."""
    monkeypatch.delenv("G2VEC_EVAL_GRID", raising=False)
    monkeypatch.delenv("G2VEC_EVAL_LDS", raising=False)
    genes, offs, labels = ke.cbow_pathset()
    P = labels.numel()
    s, p_split, inv_b = _s_table(zero=zero_s), 1500, 1 / 1500
    ref = ke.cbow_scalar_ref64(s, genes, offs, labels, inv_b)
    ca, da = _eval_counts(s, genes, offs, labels, p_split, inv_b, P)
    cb, db = _eval_counts(s, genes, offs, labels, p_split, inv_b, P, scan=True)
    _check_eval(cb, db, ref, p_split, inv_b)
    assert torch.equal(ca, cb)
    assert torch.equal(da, db)


@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("hidden", [64, 128, 256, 512, 1024])
def test_cbow_fwd_general_exact(hidden, dtype, act):
    """Row-gather forward, every HPL and weight format: W = k/8 with
    |k| <= 2 is exact in bf16 and fp16 too, so H is bitwise equal to fp64
    and `correct` agrees on EVERY path (no 99 % rule), linear and ReLU."""
    genes, offs, labels = ke.cbow_pathset()
    gen = torch.Generator().manual_seed(hidden)
    W = ke.dyadic(gen, (ke.CBOW_G, hidden), 2)
    who = ke.dyadic(gen, (hidden,), 4)
    inv_b = 1 / 500
    H, loss, correct, dO = ke.cbow_general_ref64(W, who, genes, offs, labels,
                                                 inv_b, act=act)
    Wd = W.to(DEV)
    if dtype != "fp32":
        Wd = (Wd.bfloat16() if dtype == "bf16" else Wd.half()).contiguous()
        assert torch.equal(Wd.float().cpu(), W)        # format holds k/8
    lg, cg, dg, Hg = ops.cbow_fwd(Wd, *_dev(who, genes, offs, labels), inv_b,
                                  True, act=act)
    print("loss err", _max_err(lg, loss), "dO err", _max_err(dg, dO))
    assert ke.bitwise_equal(Hg, H)                     # pre-activation
    assert ke.bitwise_equal(cg, correct)
    assert _max_err(lg, loss) <= 1e-5
    assert _max_err(dg, dO) <= ke.dO_tol(inv_b)


# ====================================================== segment kernels
def _int_dO(seed=5):
    gen = torch.Generator().manual_seed(seed)
    return torch.randint(-8, 9, (ke.SEG_P,), generator=gen).float()


@pytest.mark.parametrize("slabs", [False, True])
def test_scatter_dO_segment_edges_exact(slabs):
    """Gene segments of 1, 63..65, 255..257, 511..513 and a 5000-instance
    hub (the 4-way unrolled main loop and its tail), integer dO: bitwise
    equal to fp64, single-pass and slab-blocked; absent genes exactly 0."""
    genes, offs = ke.segment_pathset()
    dO = _int_dO()
    ref = ke.scatter_ref64(genes, offs, dO, ke.SEG_G)
    g, o, d = _dev(genes, offs, dO)
    orig = ops.SLAB_BYTES
    try:
        if slabs:
            ops.SLAB_BYTES = 4 * 1000            # 6 slabs of 1000 paths
        plan = ops.build_scatter_plan(g, o, ke.SEG_G)
        c = ops.scatter_dO(g, o, d, ke.SEG_G, plan)
    finally:
        ops.SLAB_BYTES = orig
    assert (plan.slab_seg_ptr is not None) == slabs
    if slabs:
        assert len(plan.slab_seg_ptr) == 7
    assert ke.bitwise_equal(c, ref)
    assert float(c[11]) == 0.0 and float(c[ke.SEG_G - 1]) == 0.0


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("h", [64, 1024])
def test_cbow_bwd_rows_segment_edges_exact(h, relu):
    """Same path set through cbow_bwd_rows (HPL 1 and 16), linear and with
    the ReLU mask from H_pre (zeros and -0.0 included: masked out)."""
    genes, offs = ke.segment_pathset()
    dO = _int_dO(6)
    gen = torch.Generator().manual_seed(h)
    who = ke.dyadic(gen, (h,), 8)
    H = None
    if relu:
        H = torch.randn(ke.SEG_P, h, generator=gen)
        H[torch.rand(ke.SEG_P, h, generator=gen) < 0.05] = 0.0
        H[torch.rand(ke.SEG_P, h, generator=gen) < 0.05] = -0.0
    ref = ke.bwd_rows_ref64(who, genes, offs, dO, ke.SEG_G, H_pre=H)
    dW = ops.cbow_bwd_rows(*_dev(who, genes, offs, dO), ke.SEG_G,
                           H_pre=None if H is None else H.to(DEV))
    assert ke.bitwise_equal(dW, ref)
    assert float(dW[11].abs().sum()) == 0.0
    assert float(dW[ke.SEG_G - 1].abs().sum()) == 0.0


def test_cbow_bwd_rows_refuses_slab_blocked_plan():
    """cbow_bwd_rows writes one dW row per segment, so a slab-blocked plan
    (one segment per slab and gene) would keep only a gene's last slab.
    With slabs forced, the plan it builds itself is still single-pass and
    exact, and a slab-blocked plan handed in is an error."""
    genes, offs = ke.segment_pathset()
    dO = _int_dO(7)
    who = ke.dyadic(torch.Generator().manual_seed(1), (64,), 8)
    ref = ke.bwd_rows_ref64(who, genes, offs, dO, ke.SEG_G)
    w, g, o, d = _dev(who, genes, offs, dO)
    orig = ops.SLAB_BYTES
    try:
        ops.SLAB_BYTES = 4 * 1000
        slabbed = ops.build_scatter_plan(g, o, ke.SEG_G)
        assert slabbed.slab_seg_ptr is not None
        dW = ops.cbow_bwd_rows(w, g, o, d, ke.SEG_G)
        with pytest.raises(RuntimeError, match="single-pass plan"):
            ops.cbow_bwd_rows(w, g, o, d, ke.SEG_G, plan=slabbed)
    finally:
        ops.SLAB_BYTES = orig
    assert ke.bitwise_equal(dW, ref)


# ======================================================= GEMVs and Adam
@pytest.mark.parametrize("G", [1, 7, 33000])
@pytest.mark.parametrize("h", [64, 128, 256, 512, 1024])
def test_gemv_kernels_exact(G, h):
    """Every HPL / CPT instantiation (h = 1024: gemv_rows<16>,
    gemv_cols<4>), G = 1 and 7 (fewer rows than one block's share) and
    33000 (past gemv_rows' 8192-block cap and gemv_cols' 8-rows-per-block
    regime). Dyadic W / x / c: bitwise equal to the fp64 mv."""
    gen = torch.Generator().manual_seed(G + h)
    W = ke.dyadic(gen, (G, h), 8)
    x = ke.dyadic(gen, (h,), 8)
    c = ke.dyadic(gen, (G,), 8)
    ref_rows = ke.mv_ref64(W, x)
    ref_cols = ke.mv_ref64(W.t(), c)
    Wd, xd, cd = _dev(W, x, c)
    s = torch.full((G,), -7.0, device=DEV)
    ops.gemv_rows(Wd, xd, s)
    assert ke.bitwise_equal(s, ref_rows)
    g = torch.full((h,), -7.0, device=DEV)
    ops.gemv_cols(Wd, cd, g)
    assert ke.bitwise_equal(g, ref_cols)


ADAM_SHAPES = [(1003, 64), (1003, 256), (1003, 1024), (33000, 64)]
ADAM_HP = dict(t=5, lr=0.005, b1=0.9, b2=0.999, eps=1e-8)


def _lr_t():
    return ops.tf1_lr_t(ADAM_HP["lr"], ADAM_HP["b1"], ADAM_HP["b2"],
                        ADAM_HP["t"])


def _adam_rank1_ref(W, m, v, c, who):
    grad = torch.outer(c.double(), who.double())
    return ke.adam_ref64(W, m, v, grad, _lr_t(), ADAM_HP["b1"],
                         ADAM_HP["b2"], ADAM_HP["eps"])


def _assert_adam_close(got, ref):
    errs = [_max_err(g, r) for g, r in zip(got, ref)]
    print("adam W/m/v err", errs)
    assert errs[0] <= 1e-6 and errs[1] <= 1e-7 and errs[2] <= 1e-7


@pytest.mark.parametrize("G,h", ADAM_SHAPES)
def test_adam_rank1_vs_fp64(G, h):
    """Non-square shapes (a row/column stride mix-up cannot hide) against
    an fp64 TF1-Adam reference at the project's tolerances."""
    W, m, v, c, who, _mO, _vO = ke.adam_inputs(G, h, seed=G + h)
    ref = _adam_rank1_ref(W, m, v, c, who)
    Wd, md, vd, cd, whod = _dev(W, m, v, c, who)
    ops.adam_rank1(Wd, md, vd, cd, whod, **ADAM_HP)
    _assert_adam_close((Wd, md, vd), ref)
    assert torch.equal(whod.cpu(), who)               # who is read-only here


@pytest.mark.parametrize("G,h", ADAM_SHAPES)
def test_adam_rank1_fused_vs_unfused_and_fp64(G, h):
    """Fused epoch tail: W / m / v bitwise equal to the unfused kernel;
    the in-pass gradient W^T c is exact (dyadic W and c; G = 33000 strides
    the 1024-block cap), so who / mO / vO are compared with fp64 at
    rtol 1e-6 (about 8 fp32 roundings), who with atol 1e-6 * lr_t."""
    W, m, v, c, who, mO, vO = ke.adam_inputs(G, h, seed=G + h)
    gw = ke.mv_ref64(W.t(), c)
    who_ref, mO_ref, vO_ref = ke.adam_ref64(
        who, mO, vO, gw, _lr_t(), ADAM_HP["b1"], ADAM_HP["b2"],
        ADAM_HP["eps"])
    Wa, ma, va, ca, whoa = _dev(W, m, v, c, who)
    ops.adam_rank1(Wa, ma, va, ca, whoa, **ADAM_HP)
    Wb, mb, vb, cb, whob, mOb, vOb = _dev(W, m, v, c, who, mO, vO)
    ops.adam_rank1_fused(Wb, mb, vb, cb, whob, mOb, vOb, **ADAM_HP)
    assert torch.equal(Wa, Wb) and torch.equal(ma, mb) and torch.equal(va, vb)
    _assert_adam_close((Wb, mb, vb), _adam_rank1_ref(W, m, v, c, who))

    def rel(got, ref, atol=0.0):
        err = (got.cpu().double() - ref).abs()
        print("max err / bound", float((err / (atol + 1e-6 * ref.abs()
                                                 + 1e-300)).max()))
        return bool((err <= atol + 1e-6 * ref.abs()).all())
    assert rel(mOb, mO_ref)
    assert rel(vOb, vO_ref)
    assert rel(whob, who_ref, atol=1e-6 * ke.f32(_lr_t()))


@pytest.mark.parametrize("n", [1, 255, 257, 77777])
def test_adam_dense_ragged_vs_fp64(n):
    """n not a multiple of the 256-thread block."""
    gen = torch.Generator().manual_seed(n)
    W = torch.rand(n, generator=gen) * 2 - 1
    m = (torch.rand(n, generator=gen) - 0.5) * 0.2
    v = 0.001 + torch.rand(n, generator=gen) * 0.009
    grad = torch.rand(n, generator=gen) - 0.5
    ref = ke.adam_ref64(W, m, v, grad.double(), _lr_t(), ADAM_HP["b1"],
                        ADAM_HP["b2"], ADAM_HP["eps"])
    Wd, md, vd, gd = _dev(W, m, v, grad)
    ops.adam_dense(Wd, md, vd, gd, **ADAM_HP)
    _assert_adam_close((Wd, md, vd), ref)


# The native Adam bindings validate every tensor they dereference. Each bad
# argument below is OVERSIZED or wrong-typed (never undersized, never host
# memory): these tests check that the host refuses, and a missing guard
# would still leave the launch in bounds.
GUARD_G, GUARD_H = 8, 64


def _guard_inputs():
    t = dict(zip(("W", "m", "v", "c", "who", "mO", "vO"),
                 _dev(*ke.adam_inputs(GUARD_G, GUARD_H, seed=72))))
    t["grad"] = torch.outer(t["c"], t["who"]).contiguous()
    t["lrt"] = torch.tensor([_lr_t()], dtype=torch.float32, device=DEV)
    return t


def _native_adam(fn, t, fused=False):
    hp = (ADAM_HP["b1"], ADAM_HP["b2"], ADAM_HP["eps"])
    if fn == "adam_dense":
        ops.native().adam_dense(t["W"], t["m"], t["v"], t["grad"], t["lrt"],
                                *hp)
    else:
        ops.native().adam_rank1(t["W"], t["m"], t["v"], t["c"], t["who"],
                                t["lrt"], *hp, mO=t["mO"] if fused else None,
                                vO=t["vO"] if fused else None)


def _bigger(x, shape):
    return torch.zeros(shape, dtype=x.dtype, device=x.device)


ADAM_BAD_ARGS = {
    "rank1_c_9": ("adam_rank1", False,
                  lambda t: t.update(c=_bigger(t["c"], GUARD_G + 1))),
    "rank1_who_128": ("adam_rank1", False,
                      lambda t: t.update(who=_bigger(t["who"], 2 * GUARD_H))),
    "rank1_m_9x64": ("adam_rank1", False,
                     lambda t: t.update(m=_bigger(t["m"],
                                                  (GUARD_G + 1, GUARD_H)))),
    "rank1_mO_without_vO": ("adam_rank1", True, lambda t: t.update(vO=None)),
    "rank1_mO_128": ("adam_rank1", True,
                     lambda t: t.update(mO=_bigger(t["mO"], 2 * GUARD_H))),
    "dense_m_numel_plus_1": ("adam_dense", False,
                             lambda t: t.update(
                                 m=_bigger(t["m"], GUARD_G * GUARD_H + 1))),
    "dense_v_f64": ("adam_dense", False,
                    lambda t: t.update(v=t["v"].double())),
}


@pytest.mark.parametrize("case", sorted(ADAM_BAD_ARGS))
def test_adam_bindings_reject_bad_arguments(case):
    """A mis-sized or mis-typed moment / c / who / mO is a RuntimeError from
    the host, and W, m and v are bitwise unchanged afterwards."""
    fn, fused, spoil = ADAM_BAD_ARGS[case]
    t = _guard_inputs()
    spoil(t)
    before = {k: t[k].clone() for k in ("W", "m", "v")}
    with pytest.raises(RuntimeError):
        _native_adam(fn, t, fused)
    torch.cuda.synchronize()
    for k, b in before.items():
        assert torch.equal(t[k].view(torch.uint8), b.view(torch.uint8)), k


@pytest.mark.parametrize("fn,fused", [("adam_rank1", False),
                                      ("adam_rank1", True),
                                      ("adam_dense", False)])
def test_adam_bindings_accept_good_arguments(fn, fused):
    """The same direct calls with correct 8 x 64 arguments pass the guards
    and match the fp64 TF1-Adam reference at the Adam tolerances."""
    t = _guard_inputs()
    cpu = [t[k].cpu() for k in ("W", "m", "v", "c", "who")]
    _native_adam(fn, t, fused)
    _assert_adam_close((t["W"], t["m"], t["v"]), _adam_rank1_ref(*cpu))


# ================================================================== PCC
N_GROUP = 64          # power of two: the 1 / n_group scaling is exact


@pytest.mark.parametrize("G,S", [(1, 4), (64, 64), (65, 77), (130, 288),
                                 (70, 320)])
def test_corr_gemm_exact(G, S):
    """Integer z in -8..8: C is bitwise equal to fp64 and bitwise
    symmetric. S a multiple of 4 and not, the documented maximum, and
    S = 320 (S4 = 320: exactly 160 KiB of dynamic LDS, the guard's
    maximum); G = 1, one full tile, one row past it, several tiles."""
    zt = ke.int_rows(G, S, seed=G * 1000 + S,
                     zero_row=G // 2 if G > 1 else None)
    ref = ke.corr_ref64(zt, N_GROUP)
    C = ops.corr_gemm(zt.to(DEV), N_GROUP)
    assert C.shape == (G, G)
    assert ke.bitwise_equal(C, ref)
    assert torch.equal(C, C.t())


def test_corr_gemm_rejects_first_oversized_S():
    zt = ke.int_rows(70, 321, seed=1)
    with pytest.raises(RuntimeError, match="S too large"):
        ops.corr_gemm(zt.to(DEV), N_GROUP)


@pytest.mark.parametrize("S", [1, 63, 64, 65, 288])
def test_pcc_edges_exact(S):
    """Edges over the whole gene range (highest index, self-pairs, an
    all-zero row), S below, at and above one 64-lane pass."""
    G = 130
    zt = ke.int_rows(G, S, seed=S, zero_row=17)
    idx = torch.arange(G, dtype=torch.int32)
    edges = torch.cat([
        torch.stack([idx, idx.flip(0)], 1),              # includes G-1, 0
        torch.stack([idx, idx], 1),                      # self-pairs
        torch.stack([idx, torch.full_like(idx, 17)], 1),  # zero row
        torch.stack([torch.full_like(idx, G - 1), idx], 1),
    ]).contiguous()
    ref = ke.pcc_ref64(zt, edges, N_GROUP)
    out = ops.pcc_edges(zt.to(DEV), edges.to(DEV), N_GROUP)
    assert ke.bitwise_equal(out, ref)
    assert float(out[2 * G + 17]) == 0.0


# ================================================================= bf16
def test_bf16_copy_crafted_bit_patterns():
    """Ties to even in both directions, max finite -> inf, +-0, +-inf and
    subnormals equal torch's .bfloat16() bitwise; every NaN (default,
    full payload, payload only below the bf16 cut) stays NaN."""
    fin = ke.bits_to_f32(ke.BF16_FINITE_BITS)
    got = ops.native().bf16_copy(fin.to(DEV)).cpu()
    assert torch.equal(got.view(torch.int16), fin.bfloat16().view(torch.int16))
    nan = ke.bits_to_f32(ke.BF16_NAN_BITS)
    got = ops.native().bf16_copy(nan.to(DEV)).cpu()
    print("NaN inputs ->", [hex(b & 0xFFFF) for b in
                             got.view(torch.int16).tolist()])
    assert bool(torch.isnan(got.float()).all())
    sign = (got.view(torch.int16) < 0)
    assert torch.equal(sign, nan.view(torch.int32) < 0)   # sign kept


# ======================================= argument guards of the older ops
# A CSR pointer one short, a split outside [0, P] or a table of the wrong
# rank used to reach the kernel and be indexed out of bounds. The smallest
# real shapes: every refused call would run a handful of threads if let in.
NG_P, NG_L, NG_G, NG_H, NG_S, NG_E = 4, 3, 8, 64, 8, 4
NG_INV_B = 1.0 / NG_P


def _ng_cpu():
    gen = torch.Generator().manual_seed(91)
    genes = torch.randint(0, NG_G, (NG_P * NG_L,), generator=gen).int()
    offs = torch.arange(0, NG_P * NG_L + 1, NG_L, dtype=torch.int32)
    plan = ops.build_scatter_plan(genes, offs, NG_G)
    return dict(
        genes=genes, offs=offs, labels=(torch.arange(NG_P) % 2).float(),
        pathid=torch.repeat_interleave(
            torch.arange(NG_P, dtype=torch.int32), NG_L),
        s=ke.dyadic(gen, (NG_G,), 8), W=ke.dyadic(gen, (NG_G, NG_H), 8),
        who=ke.dyadic(gen, (NG_H,), 8), cvec=ke.dyadic(gen, (NG_G,), 8),
        dOin=torch.randint(-8, 9, (NG_P,), generator=gen).float(),
        inst_path=plan.inst_path, seg_start=plan.seg_start,
        seg_gene=plan.seg_gene,
        zt=ke.int_rows(NG_G, NG_S, seed=92),
        edge_idx=torch.randint(0, NG_G, (NG_E, 2), generator=gen).int())


def _ng_inputs():
    """The good arguments on the GPU plus sentinel-filled outputs (dO two
    longer than P, so p_split = P + 1 meets the p_split guard first)."""
    t = {k: v.to(DEV) for k, v in _ng_cpu().items()}
    t.update(p_split=2, cap=2)
    for name, shape in (("counts", 2), ("dO", NG_P + 2), ("c", NG_G),
                        ("piece", NG_P * 2), ("out_rows", NG_G),
                        ("out_cols", NG_H)):
        t[name] = torch.full((shape,), -7.0, device=DEV)
    return t


NG_OPS = {
    "fwd_scalar": lambda n, t: n.cbow_fwd_scalar(
        t["s"], t["genes"], t["offs"], t["labels"], NG_INV_B, True),
    "eval_counts": lambda n, t: n.cbow_eval_counts_(
        t["s"], t["genes"], t["offs"], t["labels"], t["p_split"],
        t["counts"], dO=t["dO"], inv_b=NG_INV_B),
    "eval_scan": lambda n, t: n.cbow_eval_scan_(
        t["s"], t["genes"], t["pathid"], t["offs"], t["labels"],
        t["p_split"], t["cap"], t["piece"], t["counts"], dO=t["dO"],
        inv_b=NG_INV_B),
    "scatter": lambda n, t: n.scatter_dO_det_(
        t["inst_path"], t["seg_start"], t["seg_gene"], t["dOin"], t["c"]),
    "bwd_rows": lambda n, t: n.cbow_bwd_rows(
        t["who"], t["inst_path"], t["seg_start"], t["seg_gene"], t["dOin"],
        NG_G),
    "cbow_fwd": lambda n, t: n.cbow_fwd(
        t["W"], t["who"], t["genes"], t["offs"], t["labels"], NG_INV_B, True),
    "gemv_rows": lambda n, t: n.gemv_rows_(t["W"], t["who"], t["out_rows"]),
    "gemv_cols": lambda n, t: n.gemv_cols_(t["W"], t["cvec"], t["out_cols"]),
    "pcc_edges": lambda n, t: n.pcc_edges(t["zt"], t["edge_idx"], N_GROUP),
    "corr_gemm": lambda n, t: n.corr_gemm(t["zt"], N_GROUP),
}


def _short(name):
    return lambda t: t.update({name: t[name][:-1].contiguous()})


def _long(name):
    return lambda t: t.update({name: torch.cat([t[name], t[name][-1:]])})


def _set(name, value):
    return lambda t: t.update({name: value})


def _reshaped(name, *shape):
    return lambda t: t.update({name: t[name].reshape(*shape)})


_W_1D = _reshaped("W", -1)
_W_3D = _reshaped("W", 2, NG_G // 2, NG_H)

# case -> (op, what to break, the guard's message)
NG_BAD_ARGS = {
    **{f"{op}_offs_{kind}": (op, f("offs"), "offs must have")
       for op in ("fwd_scalar", "eval_counts", "eval_scan", "cbow_fwd")
       for kind, f in (("short", _short), ("long", _long))},
    **{f"{op}_p_split_{name}": (op, _set("p_split", v), "p_split must be")
       for op in ("eval_counts", "eval_scan")
       for name, v in (("minus_1", -1), ("P_plus_1", NG_P + 1))},
    "eval_scan_pathid_short": ("eval_scan", _short("pathid"),
                               "pathid must have"),
    "scatter_seg_start_short": ("scatter", _short("seg_start"),
                                "seg_start must have"),
    "bwd_rows_seg_start_short": ("bwd_rows", _short("seg_start"),
                                 "seg_start must have"),
    **{f"{op}_W_{name}": (op, f, r"W must be \[G, h\]")
       for op in ("cbow_fwd", "gemv_rows", "gemv_cols")
       for name, f in (("1d", _W_1D), ("3d", _W_3D))},
    "cbow_fwd_who_128": ("cbow_fwd",
                         lambda t: t.update(who=_bigger(t["who"], 2 * NG_H)),
                         "who must have"),
    "pcc_edges_edge_idx_Ex3": (
        "pcc_edges",
        lambda t: t.update(edge_idx=_bigger(t["edge_idx"], (NG_E, 3))),
        "edge_idx must be"),
    "pcc_edges_edge_idx_1d": ("pcc_edges", _reshaped("edge_idx", -1),
                              "edge_idx must be"),
    "pcc_edges_zt_1d": ("pcc_edges", _reshaped("zt", -1), "zt must be"),
    "corr_gemm_zt_1d": ("corr_gemm", _reshaped("zt", -1), "zt must be"),
}


@pytest.mark.parametrize("case", sorted(NG_BAD_ARGS))
def test_older_bindings_reject_bad_arguments(case):
    """Each case breaks one argument of one op: a RuntimeError from the host
    that names the argument, with every tensor handed in (the sentinel-filled
    outputs included) bitwise unchanged and nothing allocated."""
    op, spoil, match = NG_BAD_ARGS[case]
    t = _ng_inputs()
    spoil(t)
    tensors = {k: v for k, v in t.items() if isinstance(v, torch.Tensor)}
    before = {k: v.clone() for k, v in tensors.items()}
    torch.cuda.synchronize()
    allocated = torch.cuda.memory_allocated()
    with pytest.raises(RuntimeError, match=match):
        NG_OPS[op](ops.native(), t)
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == allocated
    for k, b in before.items():
        assert torch.equal(tensors[k].view(torch.uint8),
                           b.view(torch.uint8)), k


def _ng_close(loss, correct, dO, ref):
    """The scalar-forward bounds of this file: `correct` equal, loss 1e-5,
    dO at the scaled project tolerance (exact sums, libm behind them)."""
    rl, rc, rd = ref
    assert torch.equal(correct.cpu(), rc)
    assert _max_err(loss, rl.double()) <= 1e-5
    assert _max_err(dO, rd.double()) <= ke.dO_tol(NG_INV_B)


@pytest.mark.parametrize("op", sorted(NG_OPS))
def test_older_bindings_accept_good_arguments(op):
    """The same direct calls with the good arguments pass the guards and give
    what cpu_ref gives: dyadic / integer inputs, so every sum is exact and
    all but loss and dO (expf / log1pf) are compared bitwise."""
    from g2vec_amd.ops import cpu_ref
    c, t = _ng_cpu(), _ng_inputs()
    t["counts"].zero_()          # the accumulating outputs start from zero
    t["c"].zero_()
    got = NG_OPS[op](ops.native(), t)
    scalar = cpu_ref.cbow_fwd_scalar(c["s"], c["genes"], c["offs"],
                                     c["labels"], NG_INV_B, True)
    if op == "fwd_scalar":
        _ng_close(*got, scalar)
    elif op in ("eval_counts", "eval_scan"):
        ps = t["p_split"]
        assert t["counts"].tolist() == [float(scalar[1][:ps].sum()),
                                        float(scalar[1][ps:].sum())]
        assert _max_err(t["dO"][:ps], scalar[2][:ps].double()) \
            <= ke.dO_tol(NG_INV_B)
        assert bool((t["dO"][ps:] == -7.0).all())
    elif op == "scatter":
        assert torch.equal(t["c"].cpu(), cpu_ref.scatter_dO(
            c["genes"], c["offs"], c["dOin"], NG_G))
    elif op == "bwd_rows":
        assert torch.equal(got.cpu(), cpu_ref.cbow_bwd_rows(
            c["who"], c["genes"], c["offs"], c["dOin"], NG_G))
    elif op == "cbow_fwd":
        rl, rc, rd, rH = cpu_ref.cbow_fwd(c["W"], c["who"], c["genes"],
                                          c["offs"], c["labels"], NG_INV_B,
                                          True)
        loss, correct, dO, H = got
        assert torch.equal(H.cpu(), rH)
        _ng_close(loss, correct, dO, (rl, rc, rd))
    elif op == "gemv_rows":
        assert torch.equal(t["out_rows"].cpu(), torch.mv(c["W"], c["who"]))
    elif op == "gemv_cols":
        assert torch.equal(t["out_cols"].cpu(),
                           torch.mv(c["W"].t(), c["cvec"]))
    elif op == "pcc_edges":
        assert torch.equal(got.cpu(), cpu_ref.pcc_edges(
            c["zt"], c["edge_idx"], N_GROUP))
    else:
        assert torch.equal(got.cpu(), cpu_ref.corr_gemm(c["zt"], N_GROUP))


# one op per family, its second tensor moved to another GPU
NG_OTHER_DEVICE = {
    "walks": lambda n, a, b: n.random_walks(
        a(torch.tensor([0, 1, 2], dtype=torch.int32)),
        b(torch.tensor([1, 0], dtype=torch.int32)), a(torch.ones(2)),
        a(torch.zeros(1, dtype=torch.int32)), 1, 2, 1),
    "cbow_fast": lambda n, a, b: n.cbow_fwd_scalar(
        a(torch.zeros(NG_G)), b(torch.zeros(3, dtype=torch.int32)),
        a(torch.tensor([0, 3], dtype=torch.int32)), a(torch.zeros(1)),
        1.0, False),
    "adam": lambda n, a, b: n.adam_dense(
        a(torch.zeros(4)), b(torch.zeros(4)), a(torch.zeros(4)),
        a(torch.zeros(4)), a(torch.ones(1)), 0.9, 0.999, 1e-8),
    "cbow_general": lambda n, a, b: n.cbow_fwd(
        a(torch.zeros(NG_G, NG_H)), b(torch.zeros(NG_H)),
        a(torch.zeros(3, dtype=torch.int32)),
        a(torch.tensor([0, 3], dtype=torch.int32)), a(torch.zeros(1)),
        1.0, False),
    "gemv": lambda n, a, b: n.gemv_rows_(
        a(torch.zeros(NG_G, NG_H)), b(torch.zeros(NG_H)),
        a(torch.zeros(NG_G))),
    "pcc": lambda n, a, b: n.pcc_edges(
        a(torch.zeros(NG_G, NG_S)),
        b(torch.zeros(NG_E, 2, dtype=torch.int32)), N_GROUP),
    "replicas": lambda n, a, b: n.gemv_rows_rep_(
        a(torch.zeros(2, NG_G, NG_H)), b(torch.zeros(2, NG_H)),
        a(torch.zeros(NG_G, 2))),
    "steps56": lambda n, a, b: n.row_norms_(
        a(torch.zeros(NG_G, NG_H)), b(torch.zeros(NG_G))),
    "perm": lambda n, a, b: n.col_moments_(
        a(torch.zeros(NG_S, NG_G)),
        b(torch.zeros(NG_G, dtype=torch.float64)),
        a(torch.zeros(NG_G, dtype=torch.float64))),
    "rank": lambda n, a, b: n.rank_columns_(
        a(torch.zeros(NG_S, NG_G)), b(torch.zeros(NG_S, NG_G))),
    "knn": lambda n, a, b: n.knn_topk_(
        a(torch.zeros(2, NG_H)), b(torch.zeros(NG_G, NG_H)), None, 1, 1,
        None, None, a(torch.zeros(2, 1, dtype=torch.int32)),
        a(torch.zeros(2, 1))),
}


@pytest.mark.skipif(torch.cuda.device_count() < 2,
                    reason="needs a second GPU")
@pytest.mark.parametrize("family", sorted(NG_OTHER_DEVICE))
def test_bindings_refuse_tensors_of_two_devices(family):
    """The launch hands raw pointers to the current stream: a tensor that
    lives on cuda:1 next to one on cuda:0 is refused by the host."""
    with pytest.raises(RuntimeError, match="must be on one device"):
        NG_OTHER_DEVICE[family](ops.native(), lambda x: x.to("cuda:0"),
                                lambda x: x.to("cuda:1"))
