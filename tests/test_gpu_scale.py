"""Scale tier: the HIP kernels past the 2^20-block cap of `grid_for`, past
flat element index 2^31 and past the natural slab threshold.

Every size is the smallest that enters its regime plus a small odd
remainder (scale_cases.py), so the second grid-stride sweep is ragged.
Inputs are periodic patterns built on the device; references are closed
forms of the pattern, proven equal to the fp64 references of kernel_edges.py
by the CPU twins (test_scale_cases_cpu.py) and compared here ON the device
in chunks of at most 2^26 elements, bitwise. Head / boundary / tail windows
come back to the host and meet the existing fp64 references directly.
Tolerances are the existing ones only (loss 1e-5, dO 1e-7 at inv_b = 1/500,
Adam 1e-6 / 1e-7 / 1e-7, the trunc-normal mismatch rule). No knob is
patched: these are the natural thresholds. Nothing is skipped on low memory:
an out-of-memory error is a failure. Each test prints its wall time and
peak device memory."""
import contextlib
import time

import numpy as np
import pytest
import torch

import kernel_edges as ke
import replicate_cases as rc
import scale_cases as sc
from g2vec_amd import ops
from g2vec_amd.ops import cpu_ref
from test_gpu_kernel_edges import _assert_adam_close

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GB = 1e9


@contextlib.contextmanager
def recorded(name, limit_gb):
    """Print wall time and peak device memory; hold the peak to the case's
    bound."""
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    yield
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    peak = torch.cuda.max_memory_allocated() / GB
    print(f"SCALE {name}: wall {wall:.2f} s, peak {peak:.2f} GB")
    torch.cuda.empty_cache()
    assert peak <= limit_gb, (name, peak)


def _dev(*ts):
    return tuple(t.to(DEV) for t in ts)


# ================================================================ walks
N_WALKS = sc.WALK_NODES * sc.WALK_REPS           # CAP_W + 8


def _walks(graph, sources):
    return ops.random_walks(*_dev(*graph, sources), sc.WALK_REPS,
                            sc.WALK_LEN, sc.WALK_SEED)


def test_walks_ring_closed_form_past_grid_cap():
    """n_walks = CAP_W + 8: the last two blocks' worth of walks belong to the
    second sweep. On the ring every row is [s, s+1, s+2] mod 8 with
    s = w % 8, length 3, no padding, hash of that triple."""
    with recorded("walks_ring", 5):
        src = torch.arange(sc.WALK_NODES, dtype=torch.int32)
        nodes, lengths, hashes = _walks(sc.ring_graph(), src)
        assert nodes.shape == (N_WALKS, sc.WALK_LEN) and N_WALKS > sc.CAP_W
        for lo, hi in sc.chunks(N_WALKS, sc.WALK_LEN):
            en, el, eh = sc.ring_expected(lo, hi, DEV)
            assert torch.equal(nodes[lo:hi], en), (lo, hi)
            assert torch.equal(lengths[lo:hi], el), (lo, hi)
            assert torch.equal(hashes[lo:hi], eh), (lo, hi)


@pytest.mark.parametrize("name", ["deg3", "stops"])
def test_walks_sampled_past_grid_cap(name):
    """Sampled walks (out-degree 3, integer weights 1..4; `stops` adds
    out-degree 2 and 0 so walks end early and are padded with -1):
    the 524 289-walk run of source 5 alone (below the cap) equals rows
    r * 8 + 5 of the full run bitwise, every one of the 4 194 312 rows is a
    valid non-revisiting walk, and the head / boundary / tail windows equal
    the CPU oracle."""
    with recorded(f"walks_{name}", 5):
        graph = sc.sampled_graph(name)
        src = torch.arange(sc.WALK_NODES, dtype=torch.int32)
        nodes, lengths, hashes = _walks(graph, src)
        assert nodes.shape == (N_WALKS, sc.WALK_LEN)
        one = torch.tensor([sc.WALK_SUB_SOURCE], dtype=torch.int32)
        sn, sl, sh = _walks(graph, one)
        assert sn.shape[0] == sc.WALK_REPS < sc.CAP_W
        rows = (torch.arange(sc.WALK_REPS, device=DEV) * sc.WALK_NODES
                + sc.WALK_SUB_SOURCE)
        assert torch.equal(sn, nodes[rows])
        assert torch.equal(sl, lengths[rows])
        assert torch.equal(sh, hashes[rows])
        ok = sc.walks_valid(nodes, lengths, hashes, src,
                            sc.walk_tables(*graph, DEV))
        assert all(ok.values()) and len(ok) == 7, ok
        seen = sorted(set(torch.unique(lengths).tolist()))
        assert seen == ([3] if name == "deg3" else [1, 2, 3])
        for win, (lo, hi) in sc.windows(N_WALKS, sc.CAP_W).items():
            on, ol, oh = cpu_ref.random_walks(
                *graph, src, sc.WALK_REPS, sc.WALK_LEN, sc.WALK_SEED,
                walk_ids=range(lo, hi))
            assert torch.equal(nodes[lo:hi].cpu(), on), win
            assert torch.equal(lengths[lo:hi].cpu(), ol), win
            assert torch.equal(hashes[lo:hi].cpu(), oh), win


# ================================================================== PCC
def test_pcc_edges_past_grid_cap():
    """E = CAP_W + 5 edges over 130 genes x 65 samples (two lane passes, a
    zero row): bitwise the 130 x 130 fp64 table gathered by edge."""
    E = sc.CAP_W + 5
    with recorded("pcc_edges", 5):
        zt = sc.pcc_rows()
        edges = sc.pcc_edge_list(E, DEV)
        out = ops.pcc_edges(zt.to(DEV), edges, sc.N_GROUP)
        assert out.shape == (E,)
        exp = sc.pcc_expected(edges)
        for lo, hi in sc.chunks(E):
            assert torch.equal(out[lo:hi], exp[lo:hi]), (lo, hi)
        for win, (lo, hi) in sc.windows(E, sc.CAP_W).items():
            ref = ke.pcc_ref64(zt, edges[lo:hi].cpu(), sc.N_GROUP)
            assert ke.bitwise_equal(out[lo:hi], ref), win
        assert edges[-5:].tolist() == [list(p) for p in sc.PCC_FORCED]
        assert float(out[-2]) == 0.0


# ======================================================== general CBOW
def _cbow_inputs(h):
    W, who = sc.cbow_tables(h)
    genes, offs, labels = sc.cbow_paths(0, sc.CBOW_P, DEV)
    return W.to(DEV), who.to(DEV), genes, offs, labels


def _class_of(lo, hi):
    return torch.arange(lo, hi, device=DEV) % sc.CBOW_CLASSES


def _check_loss_correct(loss, correct, h):
    _H, loss_c, correct_c, _ = sc.cbow_class_ref(h)
    cls = _class_of(0, sc.CBOW_P)
    assert torch.equal(correct, correct_c.float().to(DEV)[cls])
    err = float((loss.double() - loss_c.to(DEV)[cls]).abs().max())
    print("loss err", err)
    assert err <= 1e-5
    return cls


def _check_windows(W, who, got):
    """Head / boundary / tail rows against ke.cbow_general_ref64 itself."""
    for win, (lo, hi) in sc.windows(sc.CBOW_P, sc.CAP_W).items():
        g, o, y = sc.cbow_paths(lo, hi, "cpu")
        H, loss, correct, dO = ke.cbow_general_ref64(
            W.float().cpu(), who.cpu(), g, o, y, sc.CBOW_INV_B, act=1)
        lg, cg, dg, Hg = (None if t is None else t[lo:hi] for t in got)
        assert ke.bitwise_equal(cg, correct), win
        assert float((lg.cpu().double() - loss).abs().max()) <= 1e-5, win
        if Hg is not None:
            assert ke.bitwise_equal(Hg, H), win
            assert (float((dg.cpu().double() - dO).abs().max())
                    <= ke.dO_tol(sc.CBOW_INV_B)), win


def test_cbow_fwd_fp32_past_grid_cap_and_2g31():
    """cbow_fwd_kernel<float, 8>, P = CAP_W + 3, h = 512: row CAP_W is the
    first of the second sweep and the first whose H offset exceeds 2^31.
    H (8.6 GB) is bitwise the integer gather-sum of its path class, checked
    in chunks of 2^26 elements; `correct` bitwise; loss / dO within the
    existing tolerances of the per-class fp64 values."""
    with recorded("cbow_fwd_fp32", 12):
        W, who, genes, offs, labels = _cbow_inputs(sc.CBOW_H)
        loss, correct, dO, H = ops.cbow_fwd(W, who, genes, offs, labels,
                                            sc.CBOW_INV_B, True, act=1)
        assert H.shape == (sc.CBOW_P, sc.CBOW_H) and H.numel() > 2 ** 31
        H_c, _l, _c, dO_c = sc.cbow_class_ref()
        H_c = H_c.float().to(DEV)
        for lo, hi in sc.chunks(sc.CBOW_P, sc.CBOW_H):
            assert torch.equal(H[lo:hi], H_c[_class_of(lo, hi)]), (lo, hi)
        cls = _check_loss_correct(loss, correct, sc.CBOW_H)
        err = float((dO.double() - dO_c.to(DEV)[cls]).abs().max())
        print("dO err", err)
        assert err <= ke.dO_tol(sc.CBOW_INV_B)
        _check_windows(W, who, (loss, correct, dO, H))
        del H, H_c


def test_cbow_bwd_rows_relu_mask_past_2g31():
    """cbow_bwd_rows_det_kernel<8> reading the forward's 8.6 GB H as the
    ReLU mask (`pi * h` past 2^31 for the last rows) with the integer
    dO[p] = p % 7 - 3 and a single-pass plan: bitwise
    dW[g, j] = who[j] * sum_{p holds g} dO_p * 1[H[p, j] > 0], the sums taken
    in int64 over the path classes. Whole dO periods cancel, so the result
    is what the paths of the ragged end leave."""
    with recorded("cbow_bwd_rows", 12):
        W, who, genes, offs, labels = _cbow_inputs(sc.CBOW_H)
        H = ops.cbow_fwd(W, who, genes, offs, labels, sc.CBOW_INV_B, True,
                         act=1)[3]
        dO = sc.cbow_bwd_dO(0, sc.CBOW_P, DEV)
        plan = ops.build_scatter_plan(genes, offs, sc.PERIOD, slabs=False)
        assert plan.slab_seg_ptr is None
        assert plan.seg_gene.numel() == sc.PERIOD
        dW = ops.cbow_bwd_rows(who, genes, offs, dO, sc.PERIOD, plan=plan,
                               H_pre=H)
        ref = sc.cbow_bwd_ref(sc.CBOW_P)
        assert ke.bitwise_equal(dW, ref)
        del H


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_cbow_fwd_16bit_tables_past_grid_cap(dtype):
    """The other two weight formats of cbow_fwd_kernel at P = CAP_W + 3,
    h = 64, no H: `correct` bitwise, loss within the existing 1e-5."""
    h = 64
    with recorded(f"cbow_fwd_{dtype}", 5):
        W, who, genes, offs, labels = _cbow_inputs(h)
        Wd = (W.bfloat16() if dtype == "bf16" else W.half()).contiguous()
        assert torch.equal(Wd.float(), W)
        loss, correct, dO, H = ops.cbow_fwd(Wd, who, genes, offs, labels,
                                            sc.CBOW_INV_B, False, act=1)
        assert dO is None and H is None
        _check_loss_correct(loss, correct, h)
        _check_windows(Wd, who, (loss, correct, None, None))


# =========================================================== elementwise
ELEM_WINDOWS = sc.windows(sc.ELEM_N, sc.CAP_E, width=4096)


def test_adam_dense_past_grid_cap():
    """n = CAP_E + 257 elements of period-1021 W / m / v / grad: every
    element within the Adam tolerances of ke.adam_ref64 of its residue."""
    with recorded("adam_dense", 5):
        W, m, v, grad = (sc.tiled(sc.ELEM_N, p, DEV)
                         for p in sc.adam_patterns())
        ops.adam_dense(W, m, v, grad, **sc.ADAM_HP)
        refs = sc.adam_period_ref()
        errs = [sc.tile_max_err(g, r) for g, r in zip((W, m, v), refs)]
        print("adam W/m/v err", errs)
        assert errs[0] <= 1e-6 and errs[1] <= 1e-7 and errs[2] <= 1e-7
        assert sc.tile_equal(grad, sc.adam_patterns()[3])     # read-only
        for _win, (lo, hi) in ELEM_WINDOWS.items():
            idx = torch.arange(lo, hi) % sc.PERIOD
            _assert_adam_close([t[lo:hi] for t in (W, m, v)],
                               [r[idx] for r in refs])


def test_bf16_copy_past_grid_cap():
    """The crafted finite bit patterns and random finite floats, tiled:
    bitwise torch's .bfloat16() of the pattern."""
    with recorded("bf16_copy", 5):
        pat = sc.bf16_pattern()
        src = sc.tiled(sc.ELEM_N, pat, DEV)
        out = ops.native().bf16_copy(src)
        assert out.dtype == torch.bfloat16 and out.shape == (sc.ELEM_N,)
        assert sc.tile_equal(out, pat.bfloat16())
        assert sc.tile_equal(src, pat)                        # read-only
        for win, (lo, hi) in ELEM_WINDOWS.items():
            want = src[lo:hi].cpu().bfloat16()
            assert torch.equal(sc.as_bits(out[lo:hi].cpu()),
                               sc.as_bits(want)), win


def test_trunc_normal_past_grid_cap():
    """Element i depends on i only: the first 20 000 of the big fill are
    bitwise a 20 000-element launch, the window around CAP_E matches the CPU
    mirror under the existing mismatch rule, everything is within +-2 sigma
    and the standard deviation within the existing 5 %."""
    std = float(sc.TN_SIGMA)
    with recorded("trunc_normal", 5):
        big = torch.empty(sc.ELEM_N, dtype=torch.float32, device=DEV)
        ops.trunc_normal_(big, std, sc.TN_SEED)
        small = torch.empty(20000, dtype=torch.float32, device=DEV)
        ops.trunc_normal_(small, std, sc.TN_SEED)
        assert torch.equal(big[:20000], small)
        lo, hi = sc.TN_WINDOW
        host = torch.empty(hi - lo, dtype=torch.float32)
        cpu_ref.trunc_normal_(host, std, sc.TN_SEED, start=lo)
        mism = (big[lo:hi].cpu() - host).abs() > 1e-5
        print("trunc_normal window mismatches", int(mism.sum()))
        assert int(mism.sum()) <= max(2, (hi - lo) // 10000), int(mism.sum())
        s1 = s2 = 0.0
        worst = 0.0
        for a, b in sc.chunks(sc.ELEM_N, 1, sc.CHUNK // 4):
            x = big[a:b].double()
            s1 += float(x.sum())
            s2 += float((x * x).sum())
            worst = max(worst, float(x.abs().max()))
        assert worst <= 2 * std + 1e-7
        mean = s1 / sc.ELEM_N
        sd = np.sqrt(s2 / sc.ELEM_N - mean * mean)
        print("trunc_normal std ratio", sd / (sc.TN_STD * std))
        assert abs(sd / (sc.TN_STD * std) - 1.0) < 0.05


# ============================================================ slab plans
def test_scatter_natural_slab_plans():
    """P = 2 * 786 432 + 5 paths: build_scatter_plan switches to three slabs
    on its own. scatter_dO over them equals the fp64 reference and the
    single-pass plan bitwise; scatter_dO_rep at R = 4 (16-byte gathers) and
    R = 3 (scalar) equals the single op on each replica's column."""
    with recorded("scatter_slabs", 5):
        genes, offs = sc.slab_paths(sc.SLAB_P, DEV)
        plan = ops.build_scatter_plan(genes, offs, sc.PERIOD)
        assert plan.slab_seg_ptr is not None
        assert len(plan.slab_seg_ptr) == 4
        flat = ops.build_scatter_plan(genes, offs, sc.PERIOD, slabs=False)
        assert flat.slab_seg_ptr is None
        g_cpu, o_cpu = genes.cpu(), offs.cpu()
        dO_4 = sc.slab_dO(sc.SLAB_P, 4, DEV)
        single = []
        for r in range(4):
            col = dO_4[:, r].contiguous()
            c = ops.scatter_dO(genes, offs, col, sc.PERIOD, plan)
            ref = rc.scatter_ref64(g_cpu, o_cpu, col.cpu(), sc.PERIOD)
            assert ke.bitwise_equal(c, ref), r
            assert torch.equal(
                c, ops.scatter_dO(genes, offs, col, sc.PERIOD, flat)), r
            single.append(c)
        for R in (4, 3):
            dO_R = dO_4[:, :R].contiguous()
            c_R = ops.scatter_dO_rep(plan, dO_R, sc.PERIOD)
            assert c_R.shape == (sc.PERIOD, R)
            for r in range(R):
                assert torch.equal(rc.bits(c_R[:, r]), rc.bits(single[r])), \
                    (R, r)


# ======================================================= narrowing casts
# Oversized metadata only: each refused call would, without its guard, still
# launch in bounds (or fail to allocate). The refusal must come first, so
# device memory in use is unchanged afterwards.
def _refused(match, fn):
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    with pytest.raises(RuntimeError, match=match):
        fn()
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == before


@pytest.mark.parametrize("n_src", [0, 1])
def test_random_walks_rejects_num_repetition_past_int32(n_src):
    """num_repetition = 2^31 reaches the kernel as a 32-bit int: refused by
    name, with no sources (nothing to launch) and with one source at
    len_path 1 (the walk count itself is a fine 64-bit number)."""
    rp, ci, w = _dev(*sc.ring_graph())
    src = torch.arange(n_src, dtype=torch.int32, device=DEV)
    _refused("num_repetition",
             lambda: ops.random_walks(rp, ci, w, src, 2 ** 31, 1, 1))
    _refused("num_repetition",
             lambda: ops.random_walks(rp, ci, w, src, -1, 1, 1))
    if n_src:
        nodes, lengths, _ = ops.random_walks(rp, ci, w, src, 2, 1, 1)
        assert nodes.tolist() == [[0], [0]] and lengths.tolist() == [1, 1]


def test_corr_gemm_rejects_tile_count_past_int32():
    """G = 46 341 * 64 - 63 rows make 46 341^2 > 2^31 - 1 tiles, one block
    each: refused before the G x G output is asked for."""
    G = 46341 * 64 - 63
    zt = torch.zeros(G, 4, device=DEV)
    _refused("tiles", lambda: ops.corr_gemm(zt, sc.N_GROUP))
