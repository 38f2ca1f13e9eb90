"""CPU checks of tests/gemm_ref.py, the float64 restatement and case list behind tests/test_gpu_gemm_edges.py: the restatement
agrees with torch's own operators (matmul, einsum, conv1d with dilation) wherever one exists; the case list takes every path of
csrc/t2_gemm.hip that the ledger below names, on both kernels; a float32 evaluation of every case stays far below the bounds in the
module's metric (so no case leans on cancellation that the scale does not cover); a CPU emulation of the three precision levels
(bf16 round-to-nearest splits, the kernel's products kept) stays within their derived bounds and is strictly ordered; splitk_for
stays in its range; and, since the library loads without a GPU, t2_gemm's argument checks refuse what they must before any launch."""
import ctypes
import os
import re

import pytest
import torch
import torch.nn.functional as F

from tests import gemm_ref as G

@pytest.fixture(scope="module")
def refs():
    """{case: (desc, bufs, logical, ref64, scale)}, computed once, never modified."""
    cache = {}

    def get(name):
        if name not in cache:
            d, bufs, logical = G.make_inputs(G.CASES[name])
            cache[name] = (d, bufs, logical) + G.reference(d, bufs)
        return cache[name]
    return get


def _close(a, b):
    return float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max()))


# ---------------------------------------------------------------------------------------------------------------------------
# the restatement against torch's operators
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", list(G.LAYOUTS))
@pytest.mark.parametrize("placement", G.PLACEMENTS)
def test_reference_is_matmul_in_every_layout_and_placement(refs, layout, placement):
    d, bufs, lg, ref, scale = refs(f"B_k33_{layout}_{placement}")
    assert _close(ref[0], lg["A"][0].double() @ lg["B"][0].double())
    assert _close(scale[0], lg["A"][0].double().abs() @ lg["B"][0].double().abs())


@pytest.mark.parametrize("name", [n for n, c in G.CASES.items() if c["family"] == "D"] + ["A_tiles_9x3_batch2_splitk3"])
def test_reference_is_einsum_for_the_batch_cases(refs, name):
    d, bufs, lg, ref, scale = refs(name)
    nb = d["batch"]
    A, B = lg["A"].double().expand(nb, -1, -1), lg["B"].double().expand(nb, -1, -1)
    want = torch.einsum("bmk,bkn->bmn", A, B)
    if d["sC"] == 0:
        want = want.sum(0, keepdim=True)
    if d["accumulate"]:
        want = want + bufs["C"][G.c_index(d)].double()
    assert ref.shape == want.shape and _close(ref, want)


def _conv_weight(Bm, Ci, k):
    """B[k*Ci][Co] with K index j*Ci + ci -> Conv1d weight [Co][Ci][k]."""
    return Bm.double().t().reshape(-1, k, Ci).permute(0, 2, 1).contiguous()


def test_reference_with_overlapping_rows_is_conv1d(refs):
    d, bufs, lg, ref, _ = refs("F_overlapping_rows")
    Ci, k, Lp, nS = 16, 5, 25, 3
    x = bufs["A"][d["A"]:d["A"] + nS * Lp * Ci].double().view(nS, Lp, Ci)
    bias = bufs["bias"][d["bias"]:d["bias"] + d["N"]].double()
    want = F.conv1d(x.transpose(1, 2), _conv_weight(lg["B"][0], Ci, k), bias).transpose(1, 2)      # [3][21][Co]
    for s in range(nS):            # (the rows that straddle two samples are junk the production layout skips too)
        assert _close(ref[0, s * Lp:s * Lp + 21], want[s])


@pytest.mark.parametrize("name", ["F_tap_strided", "F_tap_strided_batch2"])
def test_reference_with_tap_strided_rows_is_dilated_conv1d(refs, name):
    d, bufs, lg, ref, _ = refs(name)
    Ci, k, dil, rows = 32, 3, 3, 137 + 6
    bias = bufs["bias"][d["bias"]:d["bias"] + d["N"]].double()
    for b in range(d["batch"]):
        x = bufs["A"][d["A"] + b * d["sA"]:d["A"] + b * d["sA"] + rows * Ci].double().view(rows, Ci)
        want = F.conv1d(x.t()[None], _conv_weight(lg["B"][0], Ci, k), bias, dilation=dil)[0].t()
        assert want.shape == ref[b].shape and _close(ref[b], want)


def test_materialised_form_has_the_same_reference(refs):
    for name in ("F_overlapping_rows", "F_tap_strided", "F_tap_strided_batch2"):
        d, bufs, lg, ref, scale = refs(name)
        d2, bufs2, _ = G.make_inputs(G.materialised(G.CASES[name], d), logical=lg)
        assert d2["a_tap_len"] == 0 and d2["lda"] >= d2["K"]
        bufs2["bias"] = bufs["bias"]
        ref2, scale2 = G.reference(d2, bufs2)
        assert torch.equal(ref, ref2) and torch.equal(scale, scale2)


def test_the_placements_of_family_b_share_their_operands(refs):
    for K in G.K_EDGES:
        for layout in G.LAYOUTS:
            lgs = [refs(f"B_k{K}_{layout}_{p}")[2] for p in G.PLACEMENTS]
            assert all(torch.equal(lgs[0][k], x[k]) for x in lgs[1:] for k in ("A", "B"))


def test_every_unread_element_of_an_input_is_nan(refs):
    """NaN directly behind (and in front of, and between the rows of) what the header says is read."""
    for name in ("B_k33_nt_vec", "B_k33_tn_off1", "D_b_interleavedB_Ef42", "F_tap_strided_batch2", "E_acc1_relu_mask"):
        d, bufs, lg, _, _ = refs(name)
        nb = d["batch"]
        for key, idx, stride in (("A", G.a_index(d), d["sA"]), ("B", G.b_index(d), d["sB"])):
            read = torch.zeros(bufs[key].numel(), dtype=torch.bool)
            for b in range(nb):
                read[d[key] + b * stride + idx] = True
            assert bool(torch.isnan(bufs[key][~read]).all()) and bool(torch.isfinite(bufs[key][read]).all())
            assert not bool(read[-1]) and not bool(read[int(read.nonzero().max()) + 1])


# ---------------------------------------------------------------------------------------------------------------------------
# coverage ledger: every class of path, the case that provides it, on both kernels
# ---------------------------------------------------------------------------------------------------------------------------
def _both(name):
    return {"split": name, "native": name}


LEDGER = [
    # ---- tile map (family A) ----
    ("fewer than 8 tiles", _both("A_tiles_3x1"), lambda p, d: p["nblk"] < 8 and p["nblk"] > 1),
    ("one tile", _both("A_tiles_1x1"), lambda p, d: p["nblk"] == 1),
    ("one row of tiles", _both("A_tiles_1x3"), lambda p, d: p["ntm"] == 1 and p["ntn"] == 3),
    ("nblk % 8 == 0, one full group", _both("A_tiles_8x1"), lambda p, d: p["nblk_mod8"] == 0 and p["groups"] == 1 and not p["last_group_partial"]),
    ("nblk % 8 != 0 with q >= 1", _both("A_tiles_9x1"), lambda p, d: p["nblk_mod8"] != 0 and p["q"] >= 1),
    ("ntm > 8 with ntn > 1, remainder 3 of 27", _both("A_tiles_9x3"), lambda p, d: p["ntm"] > 8 and p["ntn"] == 3 and p["nblk_mod8"] == 3),
    ("partial last group of 1", _both("A_tiles_9x3"), lambda p, d: p["groups"] == 2 and p["last_group"] == 1),
    ("partial last group of 3", _both("A_tiles_11x2"), lambda p, d: p["groups"] == 2 and p["last_group"] == 3 and p["ntn"] == 2),
    ("two full groups", _both("A_tiles_16x2"), lambda p, d: p["groups"] == 2 and not p["last_group_partial"] and p["nblk_mod8"] == 0),
    ("three groups, last of 1", _both("A_tiles_17x1"), lambda p, d: p["groups"] == 3 and p["last_group"] == 1),
    ("three groups, last of 3, remainder 1 of 57", _both("A_tiles_19x3"), lambda p, d: p["groups"] == 3 and p["last_group"] == 3 and p["nblk_mod8"] == 1),
    ("grid z = batch x splitk = 6", _both("A_tiles_9x3_batch2_splitk3"), lambda p, d: p["grid_z"] == 6 and p["batch"] == 2),
    # ---- load paths (family B: one interior tile, three edge tiles) ----
    ("interior tile on vector loads (FULL on the split kernel)", _both("B_k64_nt_vec"),
     lambda p, d: p["interior_tiles"] == 1 and p["edge_tiles"] == 3 and p["a_vec"] and p["b_vec"] and (p["depth"] == 32 or p["full_tiles"] == 1)),
    ("FULL for m-major operands", _both("B_k64_tn_vec"), lambda p, d: p["a_vec"] and p["b_vec"] and not d["a_kmajor"] and not d["b_kmajor"]),
    ("FULL for k-major A, m-major B", _both("B_k64_nn_vec"), lambda p, d: p["a_vec"] and p["b_vec"] and d["a_kmajor"] and not d["b_kmajor"]),
    ("scalar loads by ld, k-major", _both("B_k33_nt_exact"), lambda p, d: not p["a_vec"] and not p["b_vec"] and d["lda"] % 4 and d["ldb"] % 4),
    ("scalar loads by ld, m-major", _both("B_k33_tn_exact"), lambda p, d: not p["a_vec"] and not p["b_vec"] and d["lda"] == 133 and d["ldb"] == 131),
    ("guarded loads on an interior tile by the base alone", _both("B_k64_nt_off1"),
     lambda p, d: p["guarded_interior_tiles"] == 1 and d["lda"] % 4 == 0 and d["ldb"] % 4 == 0 and d["A"] % 4 == 1 and d["B"] % 4 == 1),
    ("the same for m-major operands", _both("B_k64_tn_off1"), lambda p, d: p["guarded_interior_tiles"] == 1 and not d["a_kmajor"]),
    ("K tail of 1 on a vector-legal row", _both("B_k33_nt_vec"), lambda p, d: p["k_tail_vec"] and p["K_mod_4"] == 1),
    ("K tail of 3 on a vector-legal row", _both("B_k47_nt_vec"), lambda p, d: p["k_tail_vec"] and p["K_mod_4"] == 3),
    ("K below 4 on a vector-legal row", _both("B_k3_nt_vec"), lambda p, d: p["k_tail_vec"] and d["K"] < 4),
    ("K = 1", _both("B_k1_nn_vec"), lambda p, d: d["K"] == 1),
    ("row tail on vector-legal m-major operands", _both("B_k33_tn_vec"), lambda p, d: p["r_tail_vec"] and d["M"] % 4 == 1 and d["N"] % 4 == 3),
    ("K one short of a tile", {"split": "B_k15_nn_vec", "native": "B_k31_nn_vec"}, lambda p, d: p["nkt"] == 1 and p["K_mod_depth"] == p["depth"] - 1),
    ("K = one tile", {"split": "B_k16_nn_vec", "native": "B_k32_nn_vec"}, lambda p, d: p["nkt"] == 1 and p["K_mod_depth"] == 0),
    ("K one past a tile", {"split": "B_k17_nn_vec", "native": "B_k33_nn_vec"}, lambda p, d: p["nkt"] == 2 and p["K_mod_depth"] == 1),
    ("even number of whole tiles", {"split": "B_k32_tn_vec", "native": "B_k64_tn_vec"}, lambda p, d: p["nkt"] == 2 and p["K_mod_depth"] == 0),
    ("odd number of tiles (the register ping-pong ends on its first set)", {"split": "B_k33_tn_vec", "native": "B_k65_tn_vec"},
     lambda p, d: p["nkt"] == 3 and p["splitk"] == 1),
    ("four tiles and a tail", {"split": "B_k65_nt_vec", "native": "C_nt_k512_splitk64_biases"}, lambda p, d: p["nkt"] >= 5),
    # ---- split-K (family C) ----
    ("per odd (>= 3)", {"split": "C_tn_k83_splitk2", "native": "C_wgrad_96x160x2100_splitk16"}, lambda p, d: p["per_odd"] and p["per"] >= 3),
    ("per even", {"split": "C_tn_k83_splitk3", "native": "C_tn_k83_splitk2"}, lambda p, d: not p["per_odd"] and p["empty_slices"] == 0),
    ("per = 1, no empty slice", {"split": "C_tn_k83_splitk6", "native": "C_tn_k83_splitk3"}, lambda p, d: p["per"] == 1 and p["empty_slices"] == 0),
    ("empty slices, per > 1", {"split": "C_tn_k83_splitk5", "native": "C_wgrad_96x160x2100_splitk16"}, lambda p, d: p["per"] > 1 and p["empty_slices"] >= 1),
    ("empty slices, per = 1", _both("C_tn_k83_splitk8"), lambda p, d: p["per"] == 1 and p["empty_slices"] >= 2),
    ("empty slices with two biases", _both("C_nt_k40_splitk4_biases"), lambda p, d: p["empty_slices"] >= 1 and d["bias"] is not None and d["bias2"] is not None),
    ("more slices than tiles (splitk = 64)", _both("C_nt_k512_splitk64_biases"), lambda p, d: p["splitk"] == 64 and p["empty_slices"] == 64 - 512 // p["depth"]),
    ("short last slice", {"split": "C_nn_k100_splitk3", "native": "C_tn_k83_splitk2"}, lambda p, d: p["short_last_slice"] and p["empty_slices"] == 0),
    ("short last slice in front of empty ones", _both("C_wgrad_96x160x2100_splitk16"), lambda p, d: p["short_last_slice"] and p["empty_slices"] >= 1),
    ("K % depth != 0 in the last slice", _both("C_tn_k83_splitk2"), lambda p, d: p["K_mod_depth"] != 0 and p["K_mod_4"] != 0),
    ("K % depth != 0, K % 4 = 0", _both("C_wgrad_512x80x900_splitk7"), lambda p, d: p["K_mod_depth"] == 4),
    ("split-K in the tn layout", _both("C_tn_k83_splitk4"), lambda p, d: not d["a_kmajor"] and not d["b_kmajor"] and p["splitk"] == 4),
    ("split-K in the nn layout", _both("C_nn_k100_splitk3"), lambda p, d: d["a_kmajor"] and not d["b_kmajor"] and p["splitk"] == 3),
    ("splitk = 2 with two biases and alpha", _both("C_nt_k83_splitk2_biases"), lambda p, d: p["splitk"] == 2 and d["bias2"] is not None and d["alpha"] == 0.5),
    ("four output tiles under split-K", _both("C_wgrad_512x80x900_splitk7"), lambda p, d: p["nblk"] == 4 and p["per_odd"]),
    # ---- batch (family D) ----
    ("broadcast A (sA = 0)", _both("D_a_broadcastA_Ef40"), lambda p, d: p["batch"] == 3 and d["sA"] == 0 and d["sB"] > 0 and p["a_vec"] and p["b_vec"]),
    ("batch interleaved in ldb", _both("D_b_interleavedB_Ef40"), lambda p, d: d["ldb"] == 3 * d["N"] and d["sB"] == d["N"] and p["b_vec"]),
    ("broadcast B (sB = 0) with accumulate = 1", _both("D_c_broadcastB_acc1_Ef40"), lambda p, d: d["sB"] == 0 and d["accumulate"] == 1 and p["batch"] == 3),
    ("batch reduced into one C by atomics", _both("D_d_reduce_Ef40"), lambda p, d: p["into_one_c"] and d["accumulate"] == 2),
    ("batch with split-K", _both("D_e_broadcastA_splitk2_Ef40"), lambda p, d: p["grid_z"] == 6 and d["sA"] == 0),
    ("sB % 4 != 0", _both("D_a_broadcastA_Ef42"), lambda p, d: d["sB"] % 4 != 0 and not p["b_vec"]),
    ("interleaved batch with sB % 4 != 0", _both("D_b_interleavedB_Ef42"), lambda p, d: d["sB"] % 4 == 2 and not p["b_vec"]),
    ("reduction with unaligned strides", _both("D_d_reduce_Ef42"), lambda p, d: p["into_one_c"] and d["sB"] % 4 != 0),
    ("vector loads lost to the batch stride alone", _both("D_a_stride_off4"),
     lambda p, d: d["ldb"] % 4 == 0 and d["B"] % 4 == 0 and d["sB"] % 4 != 0 and not p["b_vec"] and p["a_vec"]),
    # ---- epilogue (family E) ----
    ("negative alpha with a bias", _both("E_alpha_bias"), lambda p, d: d["alpha"] < 0 and d["bias"] is not None and not d["relu"]),
    ("accumulate = 1, relu, mask with ldmask > N", _both("E_acc1_relu_mask"),
     lambda p, d: d["accumulate"] == 1 and d["relu"] and d["mulmask"] is not None and d["ldmask"] == d["N"] + 5),
    ("relu with negative alpha", _both("E_relu_negative_alpha"), lambda p, d: d["alpha"] < 0 and d["relu"]),
    ("bias2 alone", _both("E_bias2_alone"), lambda p, d: d["bias"] is None and d["bias2"] is not None),
    ("dense ldc", _both("E_dense_ldc"), lambda p, d: d["ldc"] == d["N"]),
    ("ldc > N everywhere else", _both("E_alpha_bias"), lambda p, d: d["ldc"] == d["N"] + 3),
    # ---- addressing (family F) ----
    ("overlapping rows (lda < K)", _both("F_overlapping_rows"), lambda p, d: d["lda"] == 16 and d["K"] == 80 and p["a_vec"]),
    ("tap-strided rows", _both("F_tap_strided"), lambda p, d: d["a_tap_len"] == 32 and d["a_tap_stride"] == 96 and p["ntm"] == 2),
    ("tap-strided rows with a batch", _both("F_tap_strided_batch2"), lambda p, d: d["a_tap_len"] == 32 and p["batch"] == 2 and d["sB"] == 0),
]


def test_coverage_ledger():
    missing = []
    for cls, cases, pred in LEDGER:
        for kernel in G.KERNELS:
            name = cases[kernel]
            if name not in G.CASES:
                missing.append((cls, kernel, name, "no such case"))
                continue
            d = G.describe(G.CASES[name])
            if not pred(G.paths(d, kernel), d):
                missing.append((cls, kernel, name, G.paths(d, kernel)))
    assert not missing, missing


def test_case_families_are_what_the_gpu_module_runs():
    fam = lambda f: [c for c in G.CASES.values() if c["family"] == f]
    assert [(c["M"], c["N"]) for c in fam("A")][:10] == [(128 * m - 37, 128 * n - 5) for m, n in G.TILE_MAPS]
    assert all(c["K"] == 24 for c in fam("A"))
    assert len(fam("B")) == len(G.K_EDGES) * 3 * 3 and all((c["M"], c["N"]) == (133, 131) for c in fam("B"))
    assert sorted({c["K"] for c in fam("B")}) == [1, 3, 4, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65]
    assert sorted(c["splitk"] for c in fam("C") if c["layout"] == "tn" and c["K"] == 83) == [2, 3, 4, 5, 6, 8]
    assert all(c["accumulate"] == 2 and c.get("c0", "randn") == "randn" for c in fam("C"))
    assert len(fam("D")) == 11 and len(fam("E")) == 5 and len(fam("F")) == 3
    assert max(c["M"] * c["N"] for c in G.CASES.values()) == 2395 * 379


# ---------------------------------------------------------------------------------------------------------------------------
# inputs and scale are sane; the precision levels
# ---------------------------------------------------------------------------------------------------------------------------
def test_float32_evaluation_is_far_inside_the_bounds(refs):
    worst = {}
    for name in G.CASES:
        d, bufs, _, ref, scale = refs(name)
        got, _ = G.reference(d, bufs, dtype=torch.float32)
        e = G.metric(got, ref, scale)
        fam = G.CASES[name]["family"]
        if e >= worst.get(fam, (0.0, ""))[0]:
            worst[fam] = (e, name)
        assert e < G.BASE_BOUND["split"], (name, e)
    print("[gemm ref] float32 restatement, worst per family: " + ", ".join(f"{f} {e:.2e} ({n})" for f, (e, n) in sorted(worst.items())))
    # (measured 6e-8 ... 3.0e-7: float32 matmuls of K <= 2100; the figure depends on the host's BLAS, the bound above does not)


def test_precision_levels_emulated_on_the_cpu_hold_their_bounds_and_are_ordered(refs):
    worst = {0: 0.0, 1: 0.0, 2: 0.0}
    for name in G.CASES:
        d, bufs, _, ref, scale = refs(name)
        e = {}
        for prec, planes in G.PLANES.items():
            got, _ = G.reference(d, bufs, planes=planes)
            e[prec] = G.metric(got, ref, scale)
            worst[prec] = max(worst[prec], e[prec])
            assert e[prec] <= G.BASE_BOUND["split"] + G.PRECISION_EXTRA[prec], (name, prec, e)
        assert e[0] < e[1] < e[2], (name, e)
    print("[gemm ref] emulated precision levels, worst: " + ", ".join(f"{p} {e:.2e} /{G.BASE_BOUND['split'] + G.PRECISION_EXTRA[p]:.1e}"
                                                                       for p, e in worst.items()))


def test_bounds_add_one_rounding_per_atomic_add():
    d = G.describe(G.CASES["D_d_reduce_Ef40"])
    assert G.bound(d, "split") == 2e-6 + 3 * 2.0 ** -24 and G.bound(d, "native") == 5e-5 + 3 * 2.0 ** -24
    d = G.describe(G.CASES["C_nt_k512_splitk64_biases"])
    assert G.bound(d, "split") == 2e-6 + 64 * 2.0 ** -24
    d = G.describe(G.CASES["D_e_broadcastA_splitk2_Ef40"])
    assert G.bound(d, "split") == 2e-6 + 2 * 2.0 ** -24
    d = G.describe(G.CASES["E_alpha_bias"])
    assert G.bound(d, "split", 1) == 2e-6 + 3 * 2.0 ** -16 and G.bound(d, "split", 2) == 2e-6 + 2.0 ** -7 and G.bound(d, "native") == 5e-5


def test_splitk_for_stays_in_its_range():
    from tacotron2_amd.engine import splitk_for
    shapes = {(c["M"], c["N"], c["K"]) for c in G.CASES.values()}
    txt = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r01_gemm_shapes.txt")).read()
    prof = {tuple(int(v) for v in m) for m in re.findall(r"M=\s*(\d+)\s+N=\s*(\d+)\s+K=\s*(\d+)", txt)}
    assert len(prof) >= 10
    for M, N, K in sorted(shapes | prof):
        sk = splitk_for(M, N, K)
        assert 1 <= sk <= max(1, min(-(-K // 32) // 4, 64)), (M, N, K, sk)
    for (Mo, Ni, R), sk in G.WGRADS.items():
        assert splitk_for(Mo, Ni, R) == sk, (Mo, Ni, R)


# ---------------------------------------------------------------------------------------------------------------------------
# argument checks (no launch: the library loads and refuses without a GPU, as tests/test_abi.py shows)
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from tacotron2_amd import _lib, build
    build.build(verbose=False)
    return _lib.lib()


@pytest.mark.parametrize("name,overrides,words", G.REJECTIONS, ids=[r[0] for r in G.REJECTIONS])
def test_t2_gemm_refuses_bad_arguments(lib, name, overrides, words):
    from tacotron2_amd import _lib
    A, B, C, extra = (torch.full((16384,), float(i)) for i in range(4))
    g = G.rejected_call(_lib.make, overrides, A, B, C, extra)
    assert lib.t2_gemm(ctypes.addressof(g), None) == 1                  # T2_ERR_ARG
    msg = lib.t2_last_error().decode()
    assert "t2_gemm" in msg and words in msg, msg
    with pytest.raises(_lib.T2Error, match=r"rc=1"):
        _lib.call("t2_gemm", g, None)
    assert all(bool((t == float(i)).all()) for i, t in enumerate((A, B, C, extra)))
