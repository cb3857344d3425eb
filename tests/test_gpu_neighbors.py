"""Nearest-gene queries on the GPU: knn_tile_kernel / knn_merge_kernel held
to the assertions the CPU mirror passes in test_neighbors_cpu.py (fixtures
and reference: neighbor_cases.py), plus the launch splits, sentinel-filled
outputs and the binding's guards."""
import numpy as np
import pytest
import torch

import neighbor_cases as nc
from g2vec_amd import ops

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENT_I, SENT_V = -7, 1e30          # no index and no dot of the fixtures


@pytest.mark.parametrize("Q,G,h,k,with_q_index", nc.EXACT_CASES)
def test_exact_fixtures(Q, G, h, k, with_q_index):
    nc.check_exact(ops, nc.exact_case(Q, G, h, k, with_q_index), DEV)


@pytest.mark.parametrize("shape", nc.REAL_SHAPES)
def test_real_fixtures(shape):
    nc.check_real(ops, shape, DEV)
    print("GPU max |val - ref[idx]|",
          nc.real_error(ops, nc.real_case(*shape), DEV))


@pytest.mark.parametrize("Q,G,h,k", [(65, 1003, 68, 10), (130, 1003, 1024, 63),
                                     (65, 33000, 68, 10),
                                     (130, 33000, 128, 64)])
def test_split_invariance_exact(Q, G, h, k):
    """grid_y = 1: one block walks every candidate tile (16 or 516);
    grid_y = 16 at G = 1003: one tile per block plus the merge. Every split
    equals the reference, hence every other split, bit for bit."""
    case = nc.exact_case(Q, G, h, k, True)
    outs = []
    for gy in (1, 7, 16, 0):
        nc.check_exact(ops, case, DEV, grid_y=gy)
        outs.append(nc.run_knn(ops, case, DEV, k, gy))
    outs.append(nc.run_knn(ops, case, DEV, k, 0))            # run to run
    for idx, val in outs[1:]:
        assert torch.equal(idx, outs[0][0])
        assert torch.equal(val.view(torch.int32), outs[0][1].view(torch.int32))


@pytest.mark.parametrize("shape", nc.REAL_SHAPES[1:])
def test_split_invariance_real(shape):
    """Real values: bitwise equal idx / val for every split and run to run."""
    case = nc.real_case(*shape)
    k = shape[3]
    ref = nc.run_knn(ops, case, DEV, k, 1)
    for gy in (7, 16, 0, 0):
        idx, val = nc.run_knn(ops, case, DEV, k, gy)
        assert torch.equal(idx, ref[0])
        assert torch.equal(val.view(torch.int32), ref[1].view(torch.int32))


def test_split_invariance_g33000_real():
    """516 candidate tiles of real values, so that lists keep changing deep
    into a block's walk: splits and repeats agree bitwise, and the values
    are the k largest of the device's own full score matrix."""
    rng = np.random.default_rng(99)
    X = torch.from_numpy(nc.blob_rows(rng, 33000, 64)).to(DEV)
    qi = torch.arange(0, 33000, 254, dtype=torch.int32, device=DEV)   # 130
    Xq = X[qi.long()].contiguous()
    ref = ops.knn_topk(Xq, X, 10, q_index=qi, grid_y=1)
    for gy in (7, 16, 0, 0):
        idx, val = ops.knn_topk(Xq, X, 10, q_index=qi, grid_y=gy)
        assert torch.equal(idx, ref[0])
        assert torch.equal(val.view(torch.int32), ref[1].view(torch.int32))
    full = Xq.double() @ X.double().t()
    full[torch.arange(130, device=DEV), qi.long()] = -float("inf")
    top = full.topk(10, dim=1).values
    # unit rows: sum |a b| <= 1, so every score is within h * 2^-24 of the
    # f64 one, and so is every order statistic of a row
    assert (ref[1].double() - top).abs().max() <= 64 * 2.0 ** -24


def _native_call(case, **kw):
    """knn_topk_ on the fixture; kw gives k, idx and val and replaces other
    arguments."""
    nat = ops.native()
    a = dict(Xq=torch.from_numpy(case["Xq"]).to(DEV),
             X=torch.from_numpy(case["X"]).to(DEV),
             q_index=(None if case["q_index"] is None
                      else torch.from_numpy(case["q_index"]).to(DEV)),
             grid_y=0)
    a.update(kw)
    Q, G = a["Xq"].shape[0], a["X"].shape[0]
    gy = nat.knn_grid_y(Q, G, a["grid_y"]) if a["grid_y"] >= 0 else 1
    part_idx = part_val = None
    if gy > 1:
        part_idx = torch.full((Q, gy, max(a["k"], 1)), SENT_I, dtype=torch.int32,
                              device=DEV)
        part_val = torch.full((Q, gy, max(a["k"], 1)), SENT_V, device=DEV)
    a.setdefault("part_idx", part_idx)
    a.setdefault("part_val", part_val)
    nat.knn_topk_(a["Xq"], a["X"], a["q_index"], a["k"], a["grid_y"],
                  a["part_idx"], a["part_val"], a["idx"], a["val"])


@pytest.mark.parametrize("Q,G,h,k", [(65, 130, 68, 10), (65, 65, 68, 10),
                                     (65, 65, 68, 64), (1, 1, 4, 1),
                                     (65, 2, 68, 10)])
@pytest.mark.parametrize("grid_y", [1, 0])
def test_every_output_element_is_written(Q, G, h, k, grid_y):
    """Q = 65: a second query tile with one live row; G = 65: a second
    candidate tile with one live column; h = 68: a K tail of one MFMA step.
    Outputs pre-filled with a sentinel, direct write and merge."""
    for with_qi in (True, False):
        case = nc.exact_case(Q, G, h, k, with_qi)
        idx = torch.full((Q, k), SENT_I, dtype=torch.int32, device=DEV)
        val = torch.full((Q, k), SENT_V, device=DEV)
        _native_call(case, k=k, grid_y=grid_y, idx=idx, val=val)
        assert (idx != SENT_I).all() and (val != SENT_V).all()
        assert np.array_equal(idx.cpu().numpy(), case["idx"])
        assert np.array_equal(val.cpu().numpy().astype(np.float64),
                              case["val"])


def test_binding_guards_leave_outputs_untouched():
    Q, G, h, k = 65, 130, 68, 10
    case = nc.exact_case(Q, G, h, k, True)
    Xq = torch.from_numpy(case["Xq"]).to(DEV)
    X = torch.from_numpy(case["X"]).to(DEV)
    qi = torch.from_numpy(case["q_index"]).to(DEV)
    idx = torch.full((Q, k), SENT_I, dtype=torch.int32, device=DEV)
    val = torch.full((Q, k), SENT_V, device=DEV)
    wide = torch.zeros(G, h + 4, device=DEV)
    bad = [
        dict(Xq=Xq.double()), dict(X=X.half()),                 # dtypes
        dict(q_index=qi.long()), dict(q_index=qi.float()),
        dict(Xq=Xq.t().contiguous().t()),                       # contiguity
        dict(X=X.t().contiguous().t()),
        dict(Xq=Xq[:, :64].contiguous()),                       # h mismatch
        dict(Xq=Xq[:, :6].contiguous(), X=X[:, :6].contiguous()),   # h = 6
        dict(X=wide[:, 1:h + 1]),                               # misaligned,
        dict(X=wide.view(-1)[1:1 + G * h].view(G, h)),          # contiguous
        dict(k=0), dict(k=65), dict(k=-1),
        dict(q_index=qi[:-1].contiguous()),                     # shapes
        dict(q_index=qi.view(Q, 1)),
        dict(idx=idx[:-1]), dict(val=val[:, :-1].contiguous()),
        dict(idx=idx.long()), dict(val=val.double()),
        dict(idx=idx.view(-1)), dict(grid_y=-1),
        dict(Xq=Xq.cpu()), dict(X=X.cpu()), dict(q_index=qi.cpu()),
        dict(idx=idx.cpu()),
        dict(grid_y=3, part_idx=None, part_val=None),           # partials
        dict(grid_y=3, part_idx=torch.zeros(Q, 2, k, dtype=torch.int32,
                                            device=DEV)),
    ]
    good = dict(k=k, idx=idx, val=val)
    for kw in bad:
        with pytest.raises(RuntimeError):
            _native_call(case, **dict(good, **kw))
    torch.cuda.synchronize()
    assert (idx == SENT_I).all() and (val == SENT_V).all()
    _native_call(case, **good)                          # and the good call
    assert np.array_equal(idx.cpu().numpy(), case["idx"])


def test_wrapper_pads_odd_widths():
    """h = 6 and h = 67 through the wrapper: zero-padded to a multiple of 4,
    which is exact."""
    for h in (6, 67):
        case = nc.exact_case(65, 130, 68, 10, True)
        sub = dict(case, Xq=np.ascontiguousarray(case["Xq"][:, :h]),
                   X=np.ascontiguousarray(case["X"][:, :h]))
        sc = nc.ref_scores(sub["Xq"], sub["X"], sub["q_index"])
        sub["idx"], sub["val"] = nc.ref_topk(sc, 10)
        nc.check_exact(ops, sub, DEV)


def test_q_chunk_invariance():
    for shape in nc.STRICT_SHAPES:
        nc.check_q_chunk(shape, DEV)


def test_nearest_genes_cpu_equals_gpu():
    from g2vec_amd.neighbors import nearest_genes
    for shape in nc.STRICT_SHAPES:
        case = nc.real_case(*shape)
        k = shape[3]
        c = nearest_genes(case["X"], case["q_index"], k, device="cpu")
        g = nearest_genes(case["X"], case["q_index"], k, device=DEV)
        assert np.array_equal(c[0], g[0])
        assert np.array_equal(g[0], case["idx"])
        assert np.abs(c[1] - g[1]).max() <= nc.REAL_BOUND[shape]


def test_wrapper_errors():
    nc.check_wrapper_errors(ops, DEV)


def test_cosine_zero_and_twin_rows():
    nc.check_zero_row_cosine(DEV)


def test_pipeline_neighbors_table(tiny_files, tmp_path):
    nc.check_pipeline(tiny_files, tmp_path, DEV)
