"""CPU twins of test_gpu_scale.py. Each runs a builder of scale_cases.py at
a few thousand rows (same periods) and proves that the closed-form reference
equals the project's existing fp64 reference or cpu_ref op over the whole
reduced output; the exactness bounds of the FULL sizes are asserted here
too (they depend on the per-period tables only). The two cpu_ref extensions
the GPU windows need (`walk_ids`, `start`) are pinned to the plain calls."""
import numpy as np
import pytest
import torch

import kernel_edges as ke
import replicate_cases as rc
import scale_cases as sc
from g2vec_amd import ops
from g2vec_amd.ops import cpu_ref


def test_thresholds_are_the_launch_geometry():
    """grid_for caps at 2^20 blocks of 256 threads = 4 waves; the sizes are
    the cap plus a small odd remainder, so the second sweep is ragged."""
    assert sc.CAP_W == 4_194_304 and sc.CAP_E == 268_435_456
    assert sc.WALK_NODES * sc.WALK_REPS == sc.CAP_W + 8
    assert sc.CAP_W * sc.CBOW_H == 2 ** 31          # row CAP_W: first past it
    assert sc.CBOW_P * sc.CBOW_H == 2 ** 31 + 1536
    assert sc.ELEM_N == sc.CAP_E + 257
    assert sc.SLAB_PATHS == ops.SLAB_BYTES // 4 == 786_432
    assert -(-sc.SLAB_P // sc.SLAB_PATHS) == 3
    for per in (7, 13, 127, 130, 337, sc.PERIOD):
        assert 256 % per and (1 << 20) % per and sc.CAP_W % per
    w = sc.windows(sc.CBOW_P, sc.CAP_W)
    assert w["boundary"] == (sc.CAP_W - 32, sc.CBOW_P)


# ================================================================ walks
WALK_REPS_SMALL = 300


def test_ring_closed_form_equals_oracle():
    rp, ci, w = sc.ring_graph()
    src = torch.arange(sc.WALK_NODES, dtype=torch.int32)
    on, ol, oh = cpu_ref.random_walks(rp, ci, w, src, WALK_REPS_SMALL,
                                      sc.WALK_LEN, sc.WALK_SEED)
    en, el, eh = sc.ring_expected(0, sc.WALK_NODES * WALK_REPS_SMALL, "cpu")
    assert torch.equal(on, en) and torch.equal(ol, el)
    assert torch.equal(oh, eh)
    # a window of the full-size run is the same closed form
    lo, hi = sc.windows(sc.CAP_W + 8, sc.CAP_W)["boundary"]
    wn, wl, wh = cpu_ref.random_walks(rp, ci, w, src, sc.WALK_REPS,
                                      sc.WALK_LEN, sc.WALK_SEED,
                                      walk_ids=range(lo, hi))
    en, el, eh = sc.ring_expected(lo, hi, "cpu")
    assert torch.equal(wn, en) and torch.equal(wl, el)
    assert torch.equal(wh, eh)


@pytest.mark.parametrize("name", ["deg3", "stops"])
def test_walk_ids_equals_rows_of_the_plain_call(name):
    rp, ci, w = sc.sampled_graph(name)
    src = torch.arange(sc.WALK_NODES, dtype=torch.int32)
    args = (rp, ci, w, src, 40, sc.WALK_LEN, sc.WALK_SEED)
    full = cpu_ref.random_walks(*args)
    n = full[0].shape[0]
    assert n == 320
    same = cpu_ref.random_walks(*args, walk_ids=range(n))
    assert all(torch.equal(a, b) for a, b in zip(full, same))
    ids = [317, 0, 5, 5, 163, 8, 319]              # unordered, one repeated
    sub = cpu_ref.random_walks(*args, walk_ids=ids)
    assert all(torch.equal(a[ids], b) for a, b in zip(full, sub))
    none = cpu_ref.random_walks(*args, walk_ids=[])
    assert none[0].shape == (0, sc.WALK_LEN) and none[1].numel() == 0
    for bad in ([n], [-1]):
        with pytest.raises(ValueError, match="walk_ids"):
            cpu_ref.random_walks(*args, walk_ids=bad)


@pytest.mark.parametrize("name", ["deg3", "stops"])
def test_walk_validity_check_accepts_oracle_and_has_teeth(name):
    """The tensor-op check the GPU test runs over all 4 194 312 rows accepts
    every row of the oracle and rejects each kind of broken row."""
    rp, ci, w = sc.sampled_graph(name)
    deg = (rp[1:] - rp[:-1]).tolist()
    assert set(w.tolist()) <= {1.0, 2.0, 3.0, 4.0}
    assert deg == [3] * 8 if name == "deg3" else sorted(set(deg)) == [0, 2, 3]
    src = torch.arange(sc.WALK_NODES, dtype=torch.int32)
    nodes, lengths, hashes = cpu_ref.random_walks(
        rp, ci, w, src, WALK_REPS_SMALL, sc.WALK_LEN, sc.WALK_SEED)
    tables = sc.walk_tables(rp, ci, w, "cpu")
    ok = sc.walks_valid(nodes, lengths, hashes, src, tables)
    assert all(ok.values()) and len(ok) == 7, ok
    seen_lengths = sorted(set(lengths.tolist()))
    assert seen_lengths == ([3] if name == "deg3" else [1, 2, 3])
    assert int((nodes == -1).sum()) == int((sc.WALK_LEN - lengths).sum())
    # a sub-run of one source is the rows r * 8 + s of the full run
    one = torch.tensor([sc.WALK_SUB_SOURCE], dtype=torch.int32)
    sub = cpu_ref.random_walks(rp, ci, w, one, WALK_REPS_SMALL, sc.WALK_LEN,
                               sc.WALK_SEED)
    rows = torch.arange(WALK_REPS_SMALL) * sc.WALK_NODES + sc.WALK_SUB_SOURCE
    assert torch.equal(sub[0], nodes[rows]) and torch.equal(sub[2],
                                                            hashes[rows])

    def broken(**kw):
        t = dict(nodes=nodes.clone(), lengths=lengths.clone(),
                 hashes=hashes.clone())
        for k, f in kw.items():
            f(t[k])
        return sc.walks_valid(t["nodes"], t["lengths"], t["hashes"], src,
                              tables)
    full = int(torch.nonzero(lengths == 3)[0])
    assert not broken(nodes=lambda t: t.copy_(t.roll(1, 0)))["start"]
    assert not broken(nodes=lambda t: t[full].__setitem__(
        2, t[full, 0]))["no_revisit"]
    assert not broken(hashes=lambda t: t[7].add_(1))["hash"]
    assert not broken(lengths=lambda t: t[full].sub_(1))["pad"]
    assert broken(nodes=lambda t: t[3].fill_(99)) == {"range": False}
    # a walk cut short although an unvisited neighbour was left
    cut = broken(nodes=lambda t: t[full].__setitem__(2, -1),
                 lengths=lambda t: t[full].sub_(1))
    assert not cut["stop"]
    # a step along a non-edge
    a = int(nodes[full, 0])
    non_nb = next(b for b in range(8) if not tables[0][a, b] and b != a)
    assert not broken(nodes=lambda t: t[full].__setitem__(1, non_nb))["edge"]


# ================================================================== PCC
def test_pcc_table_gather_equals_fp64_reference():
    E = 5003
    zt = sc.pcc_rows()
    edges = sc.pcc_edge_list(E, "cpu")
    exp = sc.pcc_expected(edges)
    assert exp.dtype == torch.float32
    assert ke.bitwise_equal(exp, ke.pcc_ref64(zt, edges, sc.N_GROUP))
    assert torch.equal(exp, cpu_ref.pcc_edges(zt, edges, sc.N_GROUP))
    assert edges[-5:].tolist() == [list(p) for p in sc.PCC_FORCED]
    assert int(edges.max()) == sc.PCC_G - 1 and int(edges.min()) == 0
    assert len(set(edges[:, 0].tolist())) >= 127
    assert len(set(edges[:, 1].tolist())) == sc.PCC_G
    assert float(exp[-2]) == 0.0                    # the zero row's self-pair
    assert float(zt[sc.PCC_ZERO_ROW].abs().sum()) == 0.0
    # a one-off edge index is a different expected value almost everywhere
    assert float((exp[1:] != exp[:-1]).float().mean()) > 0.9


# ======================================================== general CBOW
CBOW_P_SMALL = sc.BWD_CLASSES + sc.CBOW_CLASSES + 3     # 16 339 paths


@pytest.fixture(scope="module")
def cbow_small():
    """The reduced path set and kernel_edges' fp64 forward over ALL of it."""
    W, who = sc.cbow_tables()
    genes, offs, labels = sc.cbow_paths(0, CBOW_P_SMALL, "cpu")
    full = ke.cbow_general_ref64(W, who, genes, offs, labels, sc.CBOW_INV_B,
                                 act=1)
    return W, who, genes, offs, labels, full


def test_cbow_paths_pattern(cbow_small):
    _W, _who, genes, offs, labels, _ = cbow_small
    lens = (offs[1:] - offs[:-1])
    p = torch.arange(CBOW_P_SMALL)
    assert torch.equal(lens.long(), 1 + p % 2)
    assert torch.equal(labels, (p % 2).float())
    first = genes[offs[:-1].long()].long()
    assert torch.equal(first, p % sc.PERIOD)
    odd = p[p % 2 == 1]
    second = genes[offs[:-1].long()[odd] + 1].long()
    assert bool((second != first[odd]).all())       # the two genes differ
    moved = second != (3 * odd + 1) % sc.PERIOD
    assert odd[moved].tolist() == [1531, 1531 + 2042, 1531 + 2 * 2042,
                                   1531 + 3 * 2042, 1531 + 4 * 2042,
                                   1531 + 5 * 2042, 1531 + 6 * 2042,
                                   1531 + 7 * 2042]
    # a window builder is a slice of the full builder
    lo, hi = 4001, 4072
    g2, o2, l2 = sc.cbow_paths(lo, hi, "cpu")
    assert torch.equal(g2, genes[int(offs[lo]):int(offs[hi])])
    assert torch.equal(o2, offs[lo:hi + 1] - offs[lo])
    assert torch.equal(l2, labels[lo:hi])


def test_cbow_class_reference_equals_fp64_forward(cbow_small):
    """H, loss, correct and dO of path p are those of class p % 2042."""
    *_, full = cbow_small
    cls = torch.arange(CBOW_P_SMALL) % sc.CBOW_CLASSES
    for got, ref in zip(sc.cbow_class_ref(), full):
        assert torch.equal(got[cls], ref)
    H = full[0]
    assert torch.equal(H, H.round()) and float(H.abs().max()) <= 4.0
    assert 0.2 < float((H > 0).double().mean()) < 0.6    # the mask matters
    assert 0.2 < float(full[2].mean()) < 0.8             # both outcomes


@pytest.mark.parametrize("h", [64])
def test_cbow_16bit_tables_are_exact(h):
    W, who = sc.cbow_tables(h)
    assert torch.equal(W.bfloat16().float(), W)
    assert torch.equal(W.half().float(), W)
    _H, loss, correct, _ = sc.cbow_class_ref(h)
    assert loss.shape == (sc.CBOW_CLASSES,)
    assert 0.2 < float(correct.mean()) < 0.8


def test_cbow_bwd_class_sum_equals_fp64_backward(cbow_small):
    """The int64 per-class sum equals ke.bwd_rows_ref64 over every instance
    of the reduced set; at the full size it stays below 2^24 quanta of 1/8
    per output (ke.exact_ref inside cbow_bwd_ref asserts it)."""
    _W, who, genes, offs, _labels, full = cbow_small
    dO = sc.cbow_bwd_dO(0, CBOW_P_SMALL, "cpu")
    assert sorted(set(dO.tolist())) == [-3.0, -2.0, -1.0, 0.0, 1.0, 2.0, 3.0]
    ref = ke.bwd_rows_ref64(who, genes, offs, dO, sc.PERIOD, H_pre=full[0])
    assert torch.equal(sc.cbow_bwd_ref(CBOW_P_SMALL), ref)
    big = sc.cbow_bwd_ref(sc.CBOW_P)                 # the bound, full size
    assert big.shape == (sc.PERIOD, sc.CBOW_H)
    # dO runs through -3..3 once per 7 paths, so whole periods cancel and
    # dW is what the LAST P % 14294 paths leave: the ragged end decides it
    tail = sc.cbow_bwd_ref(sc.CBOW_P % sc.BWD_CLASSES)
    assert torch.equal(big, tail)
    assert float((big != 0).double().mean()) > 0.2
    # the count of a class is what a loop over p would count
    c = np.arange(sc.BWD_CLASSES)
    n_c = CBOW_P_SMALL // sc.BWD_CLASSES + (c < CBOW_P_SMALL % sc.BWD_CLASSES)
    assert np.array_equal(
        n_c, np.bincount(np.arange(CBOW_P_SMALL) % sc.BWD_CLASSES,
                         minlength=sc.BWD_CLASSES))


# =========================================================== elementwise
ELEM_SMALL = 5003


def test_tile_helpers():
    pat = torch.arange(7.0)
    t = sc.tiled(24, pat, "cpu")
    assert t.tolist() == [float(i % 7) for i in range(24)]
    assert sc.tile_equal(t, pat)
    assert sc.tile_max_err(t, pat.double()) == 0.0
    t[23] += 0.5
    assert not sc.tile_equal(t, pat)
    assert sc.tile_max_err(t, pat.double()) == 0.5
    z = torch.zeros(9)
    assert not sc.tile_equal(-z, torch.zeros(3))     # bitwise: -0.0 != +0.0
    assert sc.chunks(10, 4, 8) == [(0, 2), (2, 4), (4, 6), (6, 8), (8, 10)]
    assert (sc.CHUNK // sc.PERIOD) * sc.PERIOD <= 1 << 26


def test_adam_period_reference_equals_fp64_reference():
    pats = sc.adam_patterns()
    W, m, v, grad = (sc.tiled(ELEM_SMALL, p, "cpu") for p in pats)
    ref = ke.adam_ref64(W, m, v, grad.double(), sc.adam_lr_t(),
                        sc.ADAM_HP["b1"], sc.ADAM_HP["b2"],
                        sc.ADAM_HP["eps"])
    idx = torch.arange(ELEM_SMALL) % sc.PERIOD
    for per, whole in zip(sc.adam_period_ref(), ref):
        assert torch.equal(per[idx], whole)
    # value ranges of test_adam_dense_ragged_vs_fp64
    assert float(pats[0].abs().max()) <= 1.0 and float(pats[1].abs().max()) <= 0.1
    assert 0.001 <= float(pats[2].min()) and float(pats[2].max()) <= 0.01
    assert float(pats[3].abs().max()) <= 0.5
    # the fp32 op sits inside the project's Adam tolerances of it, and an
    # element computed from its neighbour's inputs does not
    cpu_ref.adam_dense(W, m, v, grad, **sc.ADAM_HP)
    errs = [sc.tile_max_err(g, r) for g, r in zip((W, m, v),
                                                  sc.adam_period_ref())]
    assert errs[0] <= 1e-6 and errs[1] <= 1e-7 and errs[2] <= 1e-7, errs
    assert sc.tile_max_err(W.roll(1), sc.adam_period_ref()[0]) > 1e-3


def test_bf16_pattern_tiles():
    pat = sc.bf16_pattern()
    assert torch.equal(pat[:24], ke.bits_to_f32(ke.BF16_FINITE_BITS))
    assert bool(torch.isfinite(pat[24:]).all())
    src = sc.tiled(ELEM_SMALL, pat, "cpu")
    assert sc.tile_equal(src, pat)
    assert sc.tile_equal(src.bfloat16(), pat.bfloat16())
    assert not sc.tile_equal(src.roll(1).bfloat16(), pat.bfloat16())


def test_trunc_normal_start_is_a_slice_of_the_longer_fill():
    std = float(sc.TN_SIGMA)
    long = torch.empty(300)
    cpu_ref.trunc_normal_(long, std, sc.TN_SEED)
    part = torch.empty(100)
    cpu_ref.trunc_normal_(part, std, sc.TN_SEED, start=123)
    assert torch.equal(part, long[123:223])
    again = torch.empty(300)
    cpu_ref.trunc_normal_(again, std, sc.TN_SEED, 0)
    assert torch.equal(again, long)
    far = torch.empty(64)                            # a 2^28-scale stream id
    cpu_ref.trunc_normal_(far, std, sc.TN_SEED, start=sc.TN_WINDOW[0])
    assert bool((far.abs() <= 2 * std + 1e-7).all())
    assert not torch.equal(far, long[:64])
    assert sc.TN_WINDOW[1] - sc.TN_WINDOW[0] == 2305


# ============================================================ slab plans
SLAB_P_SMALL = 5003


def test_slab_pattern_and_reference():
    genes, offs = sc.slab_paths(SLAB_P_SMALL, "cpu")
    lens = (offs[1:] - offs[:-1]).long()
    assert torch.equal(lens, 1 + torch.arange(SLAB_P_SMALL) % 3)
    path_of = torch.repeat_interleave(torch.arange(SLAB_P_SMALL), lens)
    key = path_of * sc.PERIOD + genes.long()
    assert key.unique().numel() == key.numel()       # distinct within a path
    assert int(genes.min()) == 0 and int(genes.max()) == sc.PERIOD - 1
    dO_R = sc.slab_dO(SLAB_P_SMALL, 4, "cpu")
    assert float(dO_R.min()) == -6.0 and float(dO_R.max()) == 6.0
    assert not torch.equal(dO_R[:, 0], dO_R[:, 1])
    plan = ops.build_scatter_plan(genes, offs, sc.PERIOD)
    c_R = ops.scatter_dO_rep(plan, dO_R, sc.PERIOD)
    for r in range(4):
        col = dO_R[:, r].contiguous()
        ref = rc.scatter_ref64(genes, offs, col, sc.PERIOD)
        assert ke.bitwise_equal(cpu_ref.scatter_dO(genes, offs, col,
                                                   sc.PERIOD), ref)
        assert ke.bitwise_equal(c_R[:, r], ref)


def test_slab_full_size_sums_stay_exact():
    """The bound of the full-size case: every per-gene sum of |dO| is below
    2^24 (rc.scatter_ref64 asserts it through ke.exact_ref)."""
    genes, offs = sc.slab_paths(sc.SLAB_P, "cpu")
    dO_R = sc.slab_dO(sc.SLAB_P, 4, "cpu")
    for r in range(4):
        ref = rc.scatter_ref64(genes, offs, dO_R[:, r].contiguous(),
                               sc.PERIOD)
        assert float(ref.abs().max()) > 0.0
    forced = ops.build_scatter_plan(genes, offs, sc.PERIOD, _force_slabs=True)
    assert len(forced.slab_seg_ptr) == 4             # three slabs
    assert forced.slab_seg_ptr[-1] == forced.seg_gene.numel()
