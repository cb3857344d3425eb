"""L-group silhouettes on the GPU: row_sqnorms_kernel, cds_tile_kernel and
cds_fold_kernel held to the assertions the CPU mirror passes in
test_silhouette_cpu.py (fixtures and reference: silhouette_cases.py), plus
the launch splits, sentinel-filled outputs and the binding's guards."""
import numpy as np
import pytest
import torch

import silhouette_cases as sc
from g2vec_amd import ops

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENT = -7.0                       # no distance sum and no squared norm


@pytest.mark.parametrize("Q,G,h,k,layout", sc.EXACT_CASES)
def test_exact_fixtures(Q, G, h, k, layout):
    sc.check_exact(ops, sc.exact_case(Q, G, h, k, layout), DEV)


def test_label_layouts():
    sc.check_layout_properties(ops, DEV)


@pytest.mark.parametrize("Q,G,h,k", sc.SPLIT_CASES)
def test_splits(Q, G, h, k):
    """grid_y = 1: one block walks every candidate tile (16 or 516) and
    writes D itself; 7 and 16: partials and the fold (16 at G = 1003: one
    tile per block); 0: the automatic split."""
    sc.check_splits(ops, sc.exact_case(Q, G, h, k), DEV)


@pytest.mark.parametrize("shape", sc.REAL_SHAPES)
def test_splits_real(shape):
    """Real values: splits within 1e-12 of each other, repeats bitwise."""
    case = sc.real_case(*shape)
    ref = sc.run_sums(ops, case, DEV, 1)
    for gy in (7, 16, 0):
        D = sc.run_sums(ops, case, DEV, gy)
        assert ((D - ref).abs() <= sc.SPLIT_REL * ref).all()
        again = sc.run_sums(ops, case, DEV, gy)
        assert torch.equal(D.view(torch.int64), again.view(torch.int64))


@pytest.mark.parametrize("shape", sc.REAL_SHAPES)
def test_real_fixtures(shape):
    sc.check_real(ops, shape, DEV)


@pytest.mark.parametrize("shape", sc.REAL_SHAPES)
def test_centring_q_chunk_and_rows(shape):
    """At G = 3000 silhouette() splits the candidates over two blocks per
    query tile (partials + fold, KC = 8), and the full run has 47 query
    tiles where the 65-row subset has 2."""
    sc.check_invariances(shape, DEV)


def test_against_sklearn():
    sc.check_sklearn(DEV)


def test_cpu_equals_gpu_within_the_bound():
    from g2vec_amd.cluster_quality import silhouette
    for shape in sc.REAL_SHAPES:
        case = sc.real_case(*shape)
        c = silhouette(case["X"], case["labels"], case["k"], device="cpu")
        g = silhouette(case["X"], case["labels"], case["k"], device=DEV)
        assert np.abs(c["s"] - g["s"]).max() <= 2 * sc.REAL_BOUND_S[shape]


def _native_call(case, **kw):
    """cluster_dist_sums_ on the fixture; kw gives nq, nx and D and replaces
    other arguments."""
    nat = ops.native()
    a = dict(Xq=torch.from_numpy(case["Xq"]).to(DEV),
             X=torch.from_numpy(case["X"]).to(DEV),
             labels=torch.from_numpy(case["labels"]).to(DEV),
             q_index=torch.from_numpy(case["q_index"]).to(DEV),
             k=case["k"], grid_y=0)
    a.update(kw)
    Q, G = a["Xq"].shape[0], a["X"].shape[0]
    ok = a["grid_y"] >= 0 and 1 <= a["k"] <= 8
    gy = nat.cds_grid_y(Q, G, a["k"], a["grid_y"]) if ok else 1
    part = None
    if gy > 1:
        part = torch.full((Q, gy, a["k"]), SENT, dtype=torch.float64,
                          device=DEV)
    a.setdefault("part", part)
    nat.cluster_dist_sums_(a["Xq"], a["X"], a["labels"], a["q_index"], a["k"],
                           a["grid_y"], a["nq"], a["nx"], a["part"], a["D"])


def _outputs(Q, G, k):
    return dict(nq=torch.full((Q,), SENT, device=DEV),
                nx=torch.full((G,), SENT, device=DEV),
                D=torch.full((Q, k), SENT, dtype=torch.float64, device=DEV))


@pytest.mark.parametrize("Q,G,h,k", [(65, 130, 68, 3), (65, 65, 68, 8),
                                     (1, 130, 68, 3), (65, 2, 68, 3)])
@pytest.mark.parametrize("grid_y", [1, 0])
def test_every_output_element_is_written(Q, G, h, k, grid_y):
    """Q = 65: a second query tile with one live row; G = 65: a second
    candidate tile with one live column. Outputs pre-filled with a
    sentinel, direct write and fold; the squared norms are the f64 ones
    rounded once."""
    case = sc.exact_case(Q, G, h, k)
    out = _outputs(Q, G, k)
    _native_call(case, grid_y=grid_y, **out)
    for t in out.values():
        assert (t != SENT).all()
    assert sc.rel_err(out["D"].cpu().numpy(), case["D"]) <= sc.EXACT_REL
    want = (case["X"].astype(np.float64) ** 2).sum(axis=1)
    assert np.array_equal(out["nx"].cpu().numpy().astype(np.float64), want)
    assert torch.equal(out["nq"], out["nx"][torch.from_numpy(
        case["q_index"]).long().to(DEV)])


def test_q_index_none_and_minus_one_exclude_nothing():
    case = sc.exact_case(65, 130, 68, 3)
    dist = sc.ref_dist(case["Xq"], case["X"])
    full = sc.ref_sums(dist, case["labels"], 3, None)
    D = sc.run_sums(ops, dict(case, q_index=None), DEV).cpu().numpy()
    assert sc.rel_err(D, full) <= sc.EXACT_REL
    qi = case["q_index"].copy()
    qi[::2] = -1
    D = sc.run_sums(ops, dict(case, q_index=qi), DEV).cpu().numpy()
    want = sc.ref_sums(dist, case["labels"], 3, qi)
    assert sc.rel_err(D, want) <= sc.EXACT_REL


def test_binding_guards_leave_outputs_untouched():
    Q, G, h, k = 65, 130, 68, 3
    case = sc.exact_case(Q, G, h, k)
    Xq = torch.from_numpy(case["Xq"]).to(DEV)
    X = torch.from_numpy(case["X"]).to(DEV)
    lab = torch.from_numpy(case["labels"]).to(DEV)
    qi = torch.from_numpy(case["q_index"]).to(DEV)
    out = _outputs(Q, G, k)
    wide = torch.zeros(G, h + 4, device=DEV)
    low, high = lab.clone(), lab.clone()
    low[9] = -1
    high[11] = k
    bad = [
        dict(Xq=Xq.double()), dict(X=X.half()),                 # dtypes
        dict(labels=lab.long()), dict(labels=lab.float()),
        dict(q_index=qi.long()), dict(q_index=qi.float()),
        dict(Xq=Xq.t().contiguous().t()),                       # contiguity
        dict(X=X.t().contiguous().t()),
        dict(Xq=Xq[:, :64].contiguous()),                       # h mismatch
        dict(Xq=Xq[:, :6].contiguous(), X=X[:, :6].contiguous()),   # h = 6
        dict(X=wide.view(-1)[1:1 + G * h].view(G, h)),          # misaligned
        dict(k=0), dict(k=9), dict(k=-1),
        dict(labels=low), dict(labels=high),                    # label range
        dict(labels=lab[:-1].contiguous()), dict(labels=lab.view(G, 1)),
        dict(q_index=qi[:-1].contiguous()), dict(q_index=qi.view(Q, 1)),
        dict(D=out["D"][:-1]), dict(D=out["D"].float()),
        dict(D=out["D"].view(-1)), dict(nq=out["nq"][:-1]),
        dict(nx=out["nx"].double()), dict(grid_y=-1),
        dict(Xq=Xq.cpu()), dict(X=X.cpu()), dict(labels=lab.cpu()),
        dict(q_index=qi.cpu()), dict(D=out["D"].cpu()),         # devices
        dict(grid_y=3, part=None),                              # partials
        dict(grid_y=3, part=torch.zeros(Q, 2, k, dtype=torch.float64,
                                        device=DEV)),
    ]
    for kw in bad:
        with pytest.raises(RuntimeError):
            _native_call(case, **dict(out, **kw))
    torch.cuda.synchronize()
    for t in out.values():
        assert (t == SENT).all()
    _native_call(case, **out)                           # and the good call
    assert sc.rel_err(out["D"].cpu().numpy(), case["D"]) <= sc.EXACT_REL


def test_wrapper_pads_odd_widths():
    """h = 6 and h = 67 through the wrapper: zero-padded to a multiple of 4,
    which is exact."""
    case = sc.exact_case(65, 130, 68, 3)
    for h in (6, 67):
        sub = dict(case, Xq=np.ascontiguousarray(case["Xq"][:, :h]),
                   X=np.ascontiguousarray(case["X"][:, :h]))
        want = sc.ref_sums(sc.ref_dist(sub["Xq"], sub["X"]), case["labels"],
                           3, case["q_index"])
        D = sc.run_sums(ops, sub, DEV).cpu().numpy()
        assert sc.rel_err(D, want) <= sc.EXACT_REL


def test_wrapper_errors():
    sc.check_wrapper_errors(ops, DEV)
    case = sc.exact_case(65, 130, 68, 3)
    X = torch.from_numpy(case["X"])
    lab = torch.from_numpy(case["labels"])
    with pytest.raises(ValueError):                     # mixed devices
        ops.cluster_dist_sums(X[:4].contiguous().to(DEV), X, lab, 3)
    with pytest.raises(ValueError):
        ops.cluster_dist_sums(X[:4].contiguous().to(DEV), X.to(DEV), lab, 3)


def test_pipeline_silhouette_columns(tiny_files, tmp_path, monkeypatch):
    sc.check_pipeline(tiny_files, tmp_path, DEV, monkeypatch)
