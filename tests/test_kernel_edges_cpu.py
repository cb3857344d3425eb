"""CPU twins of test_gpu_kernel_edges.py: they validate the inputs and
references the GPU tests rely on, so a GPU mismatch is the kernel's."""
import pytest
import torch

import kernel_edges as ke
from g2vec_amd.ops import cpu_ref


@pytest.mark.parametrize("name", sorted(ke.WALK_CASES))
def test_walk_mirror_equals_oracle(name):
    """The kernel rounds the sampling target to fp32, the oracle keeps it in
    double. On every walk of the inputs the GPU tests use, that rounding
    changes no decision: the fp32-target mirror equals the oracle."""
    rp, ci, w, src, rep, L, seed, (on, ol, oh) = ke.walk_case(name)
    mn, ml, mh = ke.mirror_walks(rp, ci, w, src, rep, L, seed)
    assert torch.equal(ml, ol)
    assert torch.equal(mn, on)
    assert torch.equal(mh, oh)


def test_walk_inputs_reach_every_sampling_path():
    """The floors the GPU tests depend on, counted from the oracle."""
    rp, ci, w, src, rep, L, seed, (on, ol, _) = ke.walk_case("mixed")
    deg = rp[1:] - rp[:-1]
    assert int((deg > 256).sum()) >= 3 and int(deg[398]) == 0
    assert float(w[rp[399]:rp[400]].abs().sum()) == 0.0 and int(deg[399]) > 0
    assert all(int((deg == d).sum()) > 0 for d in (64, 65, 256, 257))
    lean, reg, chunked = ke.steps_per_sampling_path(rp, on)
    print("steps lean/register/chunked:", lean, reg, chunked,
          "mean length", float(ol.float().mean()))
    assert min(lean, reg, chunked) >= 1000
    assert int(ol[398]) == 1 and int(ol[399]) == 1     # dead ends stop at 1
    assert int(ol.max()) == L                          # output stride taken
    assert int(ke.walk_case("len200")[7][1].max()) > 128
    assert int(ke.walk_case("len512")[7][1].max()) > 256


def test_walk_comparison_detects_weight_offset_bug():
    """Teeth: reading the weight row one entry off (the wgt[j]-for-
    wgt[s + j] class of bug, invisible under all-ones weights) changes the
    walks of the non-uniform input."""
    rp, ci, w, src, rep, L, seed, (on, ol, oh) = ke.walk_case("mixed")
    sub = src[:60]
    good = ke.mirror_walks(rp, ci, w, sub, rep, L, seed)
    bad = ke.mirror_walks(rp, ci, w, sub, rep, L, seed, weight_shift=1)
    ones = torch.ones_like(w)
    good1 = ke.mirror_walks(rp, ci, ones, sub, rep, L, seed)
    bad1 = ke.mirror_walks(rp, ci, ones, sub, rep, L, seed, weight_shift=1)
    assert not torch.equal(good[0], bad[0])
    assert torch.equal(good1[0], bad1[0])     # all-ones weights cannot see it


def test_chi2_quantile_formula():
    # exact upper 1e-6 quantiles of chi-square: df 36 -> 91.50, 196 -> 304.89
    assert ke.chi2_upper_quantile(36) == pytest.approx(91.50, rel=0.01)
    assert ke.chi2_upper_quantile(196) == pytest.approx(304.89, rel=0.002)


def test_oracle_first_step_distribution():
    """The oracle itself passes the chi-square the GPU kernel is held to
    (same graph, seeds, repetitions and threshold)."""
    rp, ci, w = ke.distribution_graph()
    src = torch.tensor(ke.DIST_SOURCES, dtype=torch.int32)
    assert int(rp[src[0]]) > 0
    nodes, _, _ = cpu_ref.random_walks(rp, ci, w, src, ke.DIST_REPS, 2,
                                       ke.DIST_SEED)
    for chi2, df, zero_hits, off_row in ke.first_step_chi2(rp, ci, w, nodes):
        print("chi2", chi2, "df", df, "limit", ke.chi2_upper_quantile(df))
        assert zero_hits == 0 and off_row == 0
        assert chi2 < ke.chi2_upper_quantile(df)


def test_exactness_preconditions_hold():
    """Every exact reference the GPU module uses passes its own
    precondition (sum|terms| < 2^24 quanta, fp32-representable result)."""
    gen = torch.Generator().manual_seed(0)
    genes, offs, labels = ke.cbow_pathset()
    ke.cbow_scalar_ref64(ke.dyadic(gen, (ke.CBOW_G,), 8), genes, offs,
                         labels, 1 / 500)
    sg, so = ke.segment_pathset()
    dO = torch.randint(-8, 9, (ke.SEG_P,), generator=gen).float()
    c = ke.scatter_ref64(sg, so, dO, ke.SEG_G)
    assert float(c[11]) == 0.0 and float(c[ke.SEG_G - 1]) == 0.0
    ke.bwd_rows_ref64(ke.dyadic(gen, (64,), 8), sg, so, dO, ke.SEG_G)
    W = ke.dyadic(gen, (33000, 64), 8)
    ke.mv_ref64(W, ke.dyadic(gen, (64,), 8))
    ke.mv_ref64(W.t(), ke.dyadic(gen, (33000,), 8))
    z = ke.int_rows(70, 320, 0)
    ke.corr_ref64(z, 64)


def test_exactness_guard_trips():
    """exact_ref refuses inputs that are not exact in fp32."""
    big = torch.full((1,), float(1 << 24), dtype=torch.float64)
    with pytest.raises(AssertionError):
        ke.exact_ref(big, big, 1.0)
    third = torch.full((1,), 1.0 / 3.0, dtype=torch.float64)
    with pytest.raises(AssertionError):
        ke.exact_ref(third, third, 1.0 / 8)


def test_single_pass_plan_has_one_segment_per_gene():
    """slabs=False keeps the gene-sorted single-pass layout that
    cbow_bwd_rows needs even where the path count would slab."""
    from g2vec_amd import ops
    genes, offs = ke.segment_pathset()
    orig = ops.SLAB_BYTES
    try:
        ops.SLAB_BYTES = 4 * 1000
        slabbed = ops.build_scatter_plan(genes, offs, ke.SEG_G,
                                         _force_slabs=True)
        single = ops.build_scatter_plan(genes, offs, ke.SEG_G,
                                        _force_slabs=True, slabs=False)
    finally:
        ops.SLAB_BYTES = orig
    assert slabbed.slab_seg_ptr is not None
    assert slabbed.seg_gene.numel() > slabbed.seg_gene.unique().numel()
    assert single.slab_seg_ptr is None
    assert single.seg_gene.numel() == single.seg_gene.unique().numel()
    sizes = (single.seg_start[1:] - single.seg_start[:-1]).tolist()
    assert tuple(sizes[:11]) == ke.SEG_SIZES


def test_f32_to_bf16_rule_keeps_nan():
    """Integer model of the device f32 -> bf16 rule: the bare rounding add
    turns NaN 0x7FFFFFFF into 0x8000 (-0.0) and 0x7F800001 into 0x7F80
    (inf); with the NaN pass-through every NaN pattern stays NaN and the
    finite patterns still equal torch's rounding."""
    def rule(u, nan_guard):
        if nan_guard and (u & 0x7FFFFFFF) > 0x7F800000:
            return (u >> 16) | 0x0040
        return ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFFFFFF) >> 16

    def is_nan16(b):
        return (b & 0x7FFF) > 0x7F80
    assert rule(0x7FFFFFFF, False) == 0x8000
    assert rule(0x7F800001, False) == 0x7F80
    assert all(is_nan16(rule(u, True)) for u in ke.BF16_NAN_BITS)
    want = ke.bits_to_f32(ke.BF16_FINITE_BITS).bfloat16().view(torch.int16)
    got = [rule(u, True) for u in ke.BF16_FINITE_BITS]
    assert got == [w & 0xFFFF for w in want.tolist()]


def test_bf16_patterns_are_what_they_claim():
    fin = ke.bits_to_f32(ke.BF16_FINITE_BITS)
    nan = ke.bits_to_f32(ke.BF16_NAN_BITS)
    assert not torch.isnan(fin).any() and torch.isnan(nan).all()
    got = fin.bfloat16().view(torch.int16).tolist()
    want = {0x3F808000: 0x3F80, 0x3F818000: 0x3F82, 0x7F7FFFFF: 0x7F80,
            0x3F7F8000: 0x3F80, 0x00008000: 0x0000, 0x00018000: 0x0002}
    for bits, bf in want.items():
        assert got[ke.BF16_FINITE_BITS.index(bits)] & 0xFFFF == bf
