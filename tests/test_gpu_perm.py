"""Permutation null of the gene t-scores on the GPU: col_moments_kernel and
the two perm_t entry points held to the assertions the CPU mirror passes in
test_perm_cpu.py (fixtures and reference: perm_cases.py), plus the launch
edges and the binding's guards with sentinel-filled outputs."""
import numpy as np
import pytest
import torch

import perm_cases as pc
from g2vec_amd import ops

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.mark.parametrize("S,G,B,balanced", pc.EXACT_CASES)
def test_exact_fixtures(S, G, B, balanced):
    pc.check_exact(ops, pc.exact_case(S, G, B, balanced), DEV)


@pytest.mark.parametrize("S,G", pc.REAL_SHAPES)
def test_real_fixtures(S, G):
    pc.check_real(ops, pc.real_case(S, G), DEV)


def test_col_moments():
    case = pc.exact_case(135, 65, 65, False)
    T, Q = ops.col_moments(torch.from_numpy(case["expr"]).to(DEV))
    x = case["expr"].astype(np.float64)
    assert T.dtype == torch.float64 and Q.dtype == torch.float64
    assert np.array_equal(T.cpu().numpy(), x.sum(axis=0))
    assert np.array_equal(Q.cpu().numpy(), (x * x).sum(axis=0))
    real = pc.real_case(300, 257)["expr"]
    T, Q = ops.col_moments(torch.from_numpy(real).to(DEV))
    x = real.astype(np.float64)
    x2 = (real * real).astype(np.float64)            # the f32 product
    np.testing.assert_allclose(T.cpu().numpy(), x.sum(axis=0), rtol=0,
                               atol=1e-13 * np.abs(x).sum(axis=0).max())
    np.testing.assert_allclose(Q.cpu().numpy(), x2.sum(axis=0), rtol=1e-13)


def _native_inputs(S, G, B, balanced=True):
    case = pc.exact_case(S, G, B, balanced)
    expr = torch.from_numpy(case["expr"]).to(DEV)
    masks = torch.from_numpy(case["masks"]).to(DEV)
    T, Q = ops.col_moments(expr)
    n1 = int(case["masks"][0].sum())
    return case, expr, masks, T, Q, n1


@pytest.mark.parametrize("S,G,B", [(65, 65, 65), (5, 1, 1), (5, 65, 65),
                                   (300, 130, 200)])
def test_every_output_element_is_written(S, G, B):
    """Second tile with one live row and one live column, G = 1, and a K
    tail that is no multiple of 4: outputs pre-filled with a sentinel."""
    case, expr, masks, T, Q, n1 = _native_inputs(S, G, B)
    nat = ops.native()
    out = torch.full((B, G), -7.0, dtype=torch.float64, device=DEV)
    nat.perm_t_stats_(expr, masks, T, Q, n1, out)
    assert (out >= 0).all()
    pc.assert_rel(out.cpu().numpy(), case["stat"])
    stat_obs = torch.from_numpy(case["stat_obs"]).to(DEV)
    counts = torch.full((G,), -7, dtype=torch.int32, device=DEV)
    maxstat = torch.full((B,), -7.0, dtype=torch.float64, device=DEV)
    nat.perm_t_counts_(expr, masks, T, Q, n1, stat_obs, counts, maxstat)
    assert (counts >= 0).all() and (maxstat >= 0).all()
    thr = stat_obs * pc.TIE
    assert torch.equal(counts.long(), (out >= thr).sum(dim=0))
    assert torch.equal(maxstat, out.max(dim=1).values)


def test_binding_guards_leave_outputs_untouched():
    case, expr, masks, T, Q, n1 = _native_inputs(65, 65, 17)
    S, G, B = 65, 65, 17
    nat = ops.native()
    stat_obs = torch.from_numpy(case["stat_obs"]).to(DEV)
    out = torch.full((B, G), -7.0, dtype=torch.float64, device=DEV)
    counts = torch.full((G,), -7, dtype=torch.int32, device=DEV)
    maxstat = torch.full((B,), -7.0, dtype=torch.float64, device=DEV)
    e3, m3 = expr[:3].contiguous(), masks[:, :3].contiguous()
    bad_common = [
        dict(expr=expr.double()), dict(masks=masks.int()),      # dtypes
        dict(T=T.float()), dict(Q=Q.float()),
        dict(expr=expr.t().contiguous().t()),                   # contiguity
        dict(masks=masks.t().contiguous().t()),
        dict(masks=masks[:, :-1].contiguous()),                 # S mismatch
        dict(expr=e3, masks=m3, n1=1),                          # S = 3
        dict(n1=1), dict(n1=S - 1),                             # group of one
        dict(T=T[:-1].contiguous()),
        dict(expr=expr.cpu()),
    ]
    base = dict(expr=expr, masks=masks, T=T, Q=Q, n1=n1)
    for kw in bad_common:
        a = dict(base, **kw)
        with pytest.raises(RuntimeError):
            nat.perm_t_stats_(a["expr"], a["masks"], a["T"], a["Q"], a["n1"],
                              out)
        with pytest.raises(RuntimeError):
            nat.perm_t_counts_(a["expr"], a["masks"], a["T"], a["Q"],
                               a["n1"], stat_obs, counts, maxstat)
    for bad_out in (out.float(), out[:, :-1], out[:-1].contiguous()):
        with pytest.raises(RuntimeError):
            nat.perm_t_stats_(expr, masks, T, Q, n1, bad_out)
    for so, c, m in ((stat_obs.float(), counts, maxstat),
                     (stat_obs[:-1].contiguous(), counts, maxstat),
                     (stat_obs, counts[:-1].contiguous(), maxstat),
                     (stat_obs, counts.long(), maxstat),
                     (stat_obs, counts, maxstat[:-1].contiguous()),
                     (stat_obs, counts, maxstat.float())):
        with pytest.raises(RuntimeError):
            nat.perm_t_counts_(expr, masks, T, Q, n1, so, c, m)
    torch.cuda.synchronize()
    assert (out == -7.0).all() and (counts == -7).all()
    assert (maxstat == -7.0).all()
    # and the wrapper's own checks, on device tensors
    uneven = masks.clone()
    uneven[3, int(torch.nonzero(uneven[3] == 0)[0])] = 1
    with pytest.raises(ValueError):
        ops.perm_t_stats(expr, uneven)
    with pytest.raises(ValueError):
        ops.perm_t_counts(expr, masks, stat_obs.cpu())


def test_row_permutation_and_repeat():
    pc.check_row_permutation(ops, pc.exact_case(65, 65, 65, True), DEV)
    pc.check_row_permutation(ops, pc.real_case(135, 130), DEV)


def test_many_relabelling_tiles_per_block():
    """B large enough that a block walks several relabelling tiles (the
    launch spreads ~2048 blocks over the 16 gene tiles, so more than 128
    relabelling tiles) and keeps its exceed counts across them."""
    from g2vec_amd import scoring
    rng = np.random.default_rng(77)
    x = rng.normal(size=(65, 1024))
    labels = np.array([1] * 21 + [0] * 44)
    expr = torch.from_numpy((x - x.mean(axis=0)).astype(np.float32)).to(DEV)
    masks = torch.from_numpy(
        scoring.perm_masks(labels, 64 * 260 + 3, seed=77)).to(DEV)
    obs = torch.from_numpy((labels == 1).astype(np.uint8)[None, :]).to(DEV)
    stat_obs = ops.perm_t_stats(expr, obs)[0].contiguous()
    counts, maxstat = ops.perm_t_counts(expr, masks, stat_obs)
    stat = ops.perm_t_stats(expr, masks)
    assert torch.equal(counts.long(), (stat >= stat_obs * pc.TIE).sum(dim=0))
    assert torch.equal(maxstat, stat.max(dim=1).values)


def test_chunk_invariance():
    pc.check_chunk_invariance(pc.real_case(65, 64), DEV)


def test_planted_signal():
    pc.check_planted(DEV)


def test_pipeline_scores_table(tiny_files, tmp_path):
    pc.check_pipeline(tiny_files, tmp_path, DEV)
