"""t2_gemm restated at the level of its descriptor (include/tacotron2_amd.h, T2Gemm), in plain torch on the CPU, and the case list
of tests/test_gpu_gemm_edges.py.

reference(desc, bufs, dtype) reads a T2Gemm-shaped dict the way the header words the struct: every operand is a FLAT buffer and
desc["A"] / ["B"] / ["C"] / ["bias"] / ["bias2"] / ["mulmask"] are element offsets into it (the pointer the library is given), so
padding, overlapping rows (lda < K), tap-strided rows and misaligned bases are stated, not assumed away.  Per batch b:
    a(m, k) = A[b*sA + (a_kmajor ? m*lda + kphys(k) : k*lda + m)],  kphys(k) = (k / a_tap_len)*a_tap_stride + k % a_tap_len (or k)
    b(k, n) = B[b*sB + (b_kmajor ? n*ldb + k : k*ldb + n)]
    v_b     = alpha * sum_k a b + bias[n] + bias2[n]              (the biases once per batch GEMM, never per K slice)
    C_b     = C[b*sC + m*ldc + n];  sC = 0 with batch > 1: the batches sum into one C
    result  = mask[m*ldmask + n] * relu(accumulate ? C0 + v : v)
It returns (result, scale), both [C batches][M][N]; scale = |alpha| sum_k |a||b| + |bias| + |bias2| + |C0| (C0 only when it is
accumulated onto), summed over the batch when sC = 0, times |mask|: the size of the terms a float32 evaluation rounds, and so the
denominator of the metric  max |got - ref64| / scale  (test_split_gemm_is_as_accurate_as_f32_mfma's, extended to the epilogue).
ReLU is 1-Lipschitz, so the pre-activation's error bounds the result's and no element near the kink needs leaving out.

paths(desc, kernel) restates the conditions of the wrapper and of the two kernels (csrc/t2_gemm.hip) as a pure function: which
load path, tile map branch and K slicing a case takes.  tests/test_gemm_ref_host.py holds the ledger: every class of path must be
taken by a named case, on both kernels.

Bounds (bound()): split kernel 2e-6, native kernel 5e-5 - the figures test_split_gemm_is_as_accurate_as_f32_mfma holds the two
kernels to in this metric at K = 4096 (measured there 6.7e-7 and 1.2e-5); an atomic epilogue adds splitk * (batches into one C) *
2^-24, one rounding per atomic add of a partial sum that the scale bounds; precision "high" adds 3 * 2^-16 (the dropped products
a2b2, a1b3, a3b1 with bf16 unit roundoff 2^-8), "medium" 2^-7 (both operands rounded to bf16)."""
import torch

F64 = torch.float64
NAN = float("nan")
SENTINEL = -12345.5                    # what C's surroundings hold: rows in front of and behind the M x N region, columns N..ldc
LAYOUTS = {"nt": (1, 1), "nn": (1, 0), "tn": (0, 0)}
KERNELS = ("split", "native")         # T2Gemm.native_fp32 = 0 / 1
DEPTH = {"split": 16, "native": 32}   # SBK / BK of csrc/t2_gemm.hip
BM = BN = 128
GM = 8                                 # m-tiles per group of the tile map
BASE_BOUND = {"split": 2e-6, "native": 5e-5}
PRECISION_EXTRA = {0: 0.0, 1: 3 * 2.0 ** -16, 2: 2.0 ** -7}
PLANES = {0: 3, 1: 2, 2: 1}           # bf16 planes per operand kept by precision 0 / 1 / 2


def _cdiv(a, b):
    return (a + b - 1) // b


def _ru4(n):
    return (n + 3) // 4 * 4


# ---------------------------------------------------------------------------------------------------------------------------
# addressing
# ---------------------------------------------------------------------------------------------------------------------------
def a_index(d):
    """[M][K] element offsets of a(m, k) from the batch's A base."""
    m = torch.arange(d["M"])[:, None]
    k = torch.arange(d["K"])[None, :]
    if d["a_kmajor"]:
        if d["a_tap_len"]:
            k = (k // d["a_tap_len"]) * d["a_tap_stride"] + k % d["a_tap_len"]
        return m * d["lda"] + k
    return k * d["lda"] + m


def b_index(d):
    """[K][N] element offsets of b(k, n) from the batch's B base."""
    k = torch.arange(d["K"])[:, None]
    n = torch.arange(d["N"])[None, :]
    return n * d["ldb"] + k if d["b_kmajor"] else k * d["ldb"] + n


def c_index(d):
    """[C batches][M][N] element offsets of the result in the C buffer (offset of the base included)."""
    nb = max(1, d["batch"])
    ncb = 1 if (nb > 1 and d["sC"] == 0) else nb
    m = torch.arange(d["M"])[:, None]
    n = torch.arange(d["N"])[None, :]
    return torch.stack([d["C"] + b * d["sC"] + m * d["ldc"] + n for b in range(ncb)])


def bf16_planes(x, n):
    """x (float32) = p1 + p2 + p3 exactly, p_i = bf16 round-to-nearest-even of what is left; the first n planes."""
    out, rest = [], x.float()
    for _ in range(n):
        p = rest.bfloat16().float()
        out.append(p)
        rest = rest - p                # exact in float32
    return out


def _product(A, B, planes):
    if planes is None:
        return A @ B
    # the products the split kernel issues (csrc/t2_gemm.hip): NP = 3: a1b1, a1b2, a2b1, a2b2, a1b3, a3b1; 2: a1b1, a1b2, a2b1; 1: a1b1
    keep = {3: [(0, 0), (0, 1), (1, 0), (1, 1), (0, 2), (2, 0)], 2: [(0, 0), (0, 1), (1, 0)], 1: [(0, 0)]}[planes]
    pa, pb = bf16_planes(A, planes), bf16_planes(B, planes)
    return sum(pa[i].double() @ pb[j].double() for i, j in keep)


def reference(d, bufs, dtype=F64, planes=None):
    """(result, scale), both [C batches][M][N].  planes = 3 / 2 / 1 (float64 only): the operands split into bf16 planes and the
    products of precision 0 / 1 / 2 kept, everything else exact - the CPU emulation of T2Gemm.precision."""
    assert planes is None or dtype == F64
    nb = max(1, d["batch"])
    into_one = nb > 1 and d["sC"] == 0
    ia, ib, ic = a_index(d), b_index(d), c_index(d)
    n = torch.arange(d["N"])
    vs, ss = [], []
    for b in range(nb):
        A32 = bufs["A"][d["A"] + b * d["sA"] + ia]
        B32 = bufs["B"][d["B"] + b * d["sB"] + ib]
        v = d["alpha"] * (_product(A32, B32, planes) if planes else A32.to(dtype) @ B32.to(dtype))
        s = abs(d["alpha"]) * (A32.double().abs() @ B32.double().abs())
        for name in ("bias", "bias2"):
            if d[name] is not None:
                bb = bufs[name][d[name] + n]
                v = v + bb.to(dtype)[None, :]
                s = s + bb.double().abs()[None, :]
        vs.append(v)
        ss.append(s)
    if into_one:
        vs, ss = [sum(vs[1:], vs[0])], [sum(ss[1:], ss[0])]
    res, scale = [], []
    for b, (v, s) in enumerate(zip(vs, ss)):
        if d["accumulate"]:
            c0 = bufs["C"][ic[b]]
            v = c0.to(dtype) + v
            s = s + c0.double().abs()
        if d["relu"]:
            v = torch.relu(v)
        if d["mulmask"] is not None:
            mk = bufs["mulmask"][d["mulmask"] + torch.arange(d["M"])[:, None] * d["ldmask"] + n[None, :]]
            v = v * mk.to(dtype)
            s = s * mk.double().abs()
        res.append(v)
        scale.append(s)
    return torch.stack(res), torch.stack(scale)


def metric(got, ref, scale):
    """max |got - ref| / scale; an element whose scale is zero (a masked one, a zero operand) must be exact."""
    err = (got.double() - ref.double()).abs()
    zero = scale == 0
    if bool((err[zero] != 0).any()) or not bool(torch.isfinite(got).all()):
        return float("inf")
    return float((err[~zero] / scale[~zero]).max()) if bool((~zero).any()) else 0.0


def bound(d, kernel, precision=0):
    atomic = 0.0
    if d["accumulate"] == 2:
        nb = max(1, d["batch"])
        atomic = max(1, d["splitk"]) * (nb if d["sC"] == 0 else 1) * 2.0 ** -24
    return BASE_BOUND[kernel] + atomic + PRECISION_EXTRA[precision]


# ---------------------------------------------------------------------------------------------------------------------------
# which paths a call takes
# ---------------------------------------------------------------------------------------------------------------------------
def paths(d, kernel):
    """The wrapper's and the kernel's own conditions (csrc/t2_gemm.hip), restated.  A base offset counts as 16-byte aligned when
    it is a multiple of 4 elements (the buffers themselves are: the GPU module asserts it)."""
    depth = DEPTH[kernel]
    M, N, K = d["M"], d["N"], d["K"]
    a_vec = d["lda"] % 4 == 0 and d["A"] % 4 == 0 and d["sA"] % 4 == 0
    if d["a_tap_len"]:
        a_vec = a_vec and d["a_tap_stride"] % 4 == 0
    b_vec = d["ldb"] % 4 == 0 and d["B"] % 4 == 0 and d["sB"] % 4 == 0
    ntm, ntn = _cdiv(M, BM), _cdiv(N, BN)
    nblk = ntm * ntn
    interior = (M // BM) * (N // BN)
    splitk = max(1, d["splitk"])
    nkt = _cdiv(K, depth)
    per = _cdiv(nkt, splitk)
    nonempty = _cdiv(nkt, per)
    last_len = nkt - (nonempty - 1) * per
    nb = max(1, d["batch"])
    return dict(
        a_vec=a_vec, b_vec=b_vec, ntm=ntm, ntn=ntn, nblk=nblk, nblk_mod8=nblk % 8, q=nblk // 8,
        groups=_cdiv(ntm, GM), last_group=ntm % GM or GM, last_group_partial=ntm % GM != 0,
        interior_tiles=interior, edge_tiles=nblk - interior,
        # tiles on the FULL (unguarded 16-byte) loads: the split kernel's interior tiles with both operands vector-legal; an interior
        # tile with an operand that is not takes the guarded loads where FULL would otherwise run
        full_tiles=interior if (kernel == "split" and a_vec and b_vec) else 0,
        guarded_interior_tiles=interior if not (a_vec and b_vec) else 0,
        # a 4-element group cut short on a vector-legal operand: along K (k-major operand) or along the rows (m-major operand)
        k_tail_vec=K % 4 != 0 and ((a_vec and bool(d["a_kmajor"])) or (b_vec and bool(d["b_kmajor"]))),
        r_tail_vec=(a_vec and not d["a_kmajor"] and M % 4 != 0) or (b_vec and not d["b_kmajor"] and N % 4 != 0),
        depth=depth, nkt=nkt, splitk=splitk, per=per, per_odd=per % 2 == 1, empty_slices=splitk - nonempty,
        short_last_slice=last_len < per, K_mod_depth=K % depth, K_mod_4=K % 4,
        grid_z=nb * splitk, batch=nb, into_one_c=nb > 1 and d["sC"] == 0)


# ---------------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------------
def _extents(c):
    """(contiguous extent of A, of B) in elements: what ld must cover."""
    a_k, b_k = LAYOUTS[c["layout"]]
    return (c["K"] if a_k else c["M"]), (c["K"] if b_k else c["N"])


def describe(c):
    """Case -> T2Gemm-shaped dict with element offsets for pointers.  Defaults: ld = the extent rounded up to 4, bases 4 elements
    into their buffers (aligned, NaN in front), ldc = N + 3, C's region two rows into its buffer, dense batch strides."""
    a_k, b_k = LAYOUTS[c["layout"]]
    M, N, K = c["M"], c["N"], c["K"]
    ea, eb = _extents(c)
    lda, ldb = c.get("lda", _ru4(ea)), c.get("ldb", _ru4(eb))
    ldc = c.get("ldc", N + 3)
    nb = c.get("batch", 1)
    d = dict(A=c.get("offA", 4), B=c.get("offB", 4), C=2 * ldc, M=M, N=N, K=K, lda=lda, ldb=ldb, ldc=ldc, a_kmajor=a_k, b_kmajor=b_k,
             alpha=c.get("alpha", 1.0), bias=1 if c.get("bias") else None, bias2=2 if c.get("bias2") else None,
             mulmask=3 if c.get("ldmask") else None, ldmask=c.get("ldmask", 0), relu=c.get("relu", 0),
             accumulate=c.get("accumulate", 0), splitk=c.get("splitk", 1), batch=nb,
             sA=c.get("sA", (M if a_k else K) * lda if nb > 1 else 0), sB=c.get("sB", (N if b_k else K) * ldb if nb > 1 else 0),
             sC=c.get("sC", M * ldc if nb > 1 else 0), share_cu=c.get("share_cu", 0),
             a_tap_len=c.get("a_tap_len", 0), a_tap_stride=c.get("a_tap_stride", 0))
    return d


def _place(off, stride, idx, logical, slack=8):
    """A flat NaN buffer with logical[b] written at off + b*stride + idx: every element the header does not say is read is NaN -
    the padding columns, what lies in front of the base and what lies behind the last element."""
    nbuf = logical.shape[0]
    flat = torch.full((off + (nbuf - 1) * stride + int(idx.max()) + 1 + slack,), NAN)
    for b in range(nbuf):
        flat[off + b * stride + idx] = logical[b]
    return flat


def make_inputs(c, logical=None):
    """(desc, bufs, logical): float32 CPU buffers, seeded by the case.  logical = {"A": [A batches][M][K], "B": [B batches][K][N]}
    are the operands as matrices; given, they are placed instead of drawn (the same operands in another placement or in their
    materialised form).  C's buffer holds SENTINEL everywhere but in the M x N regions, which hold NaN (c0 = "nan": a store must
    cover them), zeros or random values (what an accumulating call adds to)."""
    d = describe(c)
    g = torch.Generator().manual_seed(c["seed"])
    nb = d["batch"]
    nA, nB = (nb if d["sA"] else 1), (nb if d["sB"] else 1)
    ia, ib, ic = a_index(d), b_index(d), c_index(d)
    M, N, K = d["M"], d["N"], d["K"]
    if logical is None:
        if c.get("overlap"):           # rows of A share elements: draw the flat signal, the matrix is a view of it
            x = torch.randn((nA - 1) * d["sA"] + int(ia.max()) + 1, generator=g)
            A = torch.stack([x[b * d["sA"] + ia] for b in range(nA)])
        else:
            A = torch.randn(nA, M, K, generator=g)
        B = torch.randn(nB, K, N, generator=g)
        logical = dict(A=A, B=B)
    else:
        g.manual_seed(c["seed"] + 7919)
    bufs = dict(A=_place(d["A"], d["sA"], ia, logical["A"]), B=_place(d["B"], d["sB"], ib, logical["B"]))
    for name in ("bias", "bias2"):
        if d[name] is not None:
            bufs[name] = _place(d[name], 0, torch.arange(N), torch.randn(1, N, generator=g))
    if d["mulmask"] is not None:       # a dropout scale mask of {0, 2}
        mk = (torch.rand(1, M, N, generator=g) > 0.5).float() * 2
        bufs["mulmask"] = _place(d["mulmask"], 0, torch.arange(M)[:, None] * d["ldmask"] + torch.arange(N)[None, :], mk)
    cbuf = torch.full((int(ic.max()) + 1 + (d["ldc"] - N) + 2 * d["ldc"],), SENTINEL)
    c0 = c.get("c0", "nan" if d["accumulate"] == 0 else "randn")
    cbuf[ic] = {"nan": lambda: torch.full(ic.shape, NAN), "zeros": lambda: torch.zeros(ic.shape),
                "randn": lambda: torch.randn(ic.shape, generator=g)}[c0]()
    bufs["C"] = cbuf
    return d, bufs, logical


def materialised(c, d):
    """The case with A's overlapping or tap-strided rows written out as a dense [M][K] matrix (im2col on the host)."""
    m = {k: v for k, v in c.items() if k not in ("lda", "a_tap_len", "a_tap_stride", "overlap", "sA")}
    m["name"] = c["name"] + "_materialised"
    if d["batch"] > 1:
        m["sA"] = d["M"] * _ru4(d["K"])
    return m


def _cases():
    cs = []

    def add(name, family, M, N, K, layout, seed, **kw):
        cs.append(dict(name=name, family=family, M=M, N=N, K=K, layout=layout, seed=seed, **kw))

    # A. tile map: store into NaN (the GPU module repeats each with accumulate = 2 into zeros)
    for i, (ntm, ntn) in enumerate(TILE_MAPS):
        add(f"A_tiles_{ntm}x{ntn}", "A", 128 * ntm - 37, 128 * ntn - 5, 24, "nt", 100 + i)
    add("A_tiles_9x3_batch2_splitk3", "A", 128 * 9 - 37, 128 * 3 - 5, 24, "nt", 120, batch=2, splitk=3, accumulate=2, c0="zeros")
    # B. K edges and load paths: one interior and three edge tiles; the three placements of one K and layout share their operands
    for K in K_EDGES:
        for li, layout in enumerate(LAYOUTS):
            base = dict(name=None, family="B", M=133, N=131, K=K, layout=layout, seed=1000 + 3 * K + li)
            ea, eb = _extents(base)
            cs.append(dict(base, name=f"B_k{K}_{layout}_vec"))
            cs.append(dict(base, name=f"B_k{K}_{layout}_exact", lda=ea, ldb=eb))
            cs.append(dict(base, name=f"B_k{K}_{layout}_off1", offA=5, offB=5))
    # C. split-K into a non-zero C
    for sk in (2, 3, 4, 5, 6, 8):
        add(f"C_tn_k83_splitk{sk}", "C", 200, 150, 83, "tn", 2000 + sk, accumulate=2, splitk=sk)
    for K, sk in ((83, 2), (40, 4), (512, 64)):
        add(f"C_nt_k{K}_splitk{sk}_biases", "C", 200, 150, K, "nt", 2100 + sk, accumulate=2, splitk=sk, bias=1, bias2=1, alpha=0.5)
    add("C_nn_k100_splitk3", "C", 200, 150, 100, "nn", 2200, accumulate=2, splitk=3)
    for (Mo, Ni, R), sk in WGRADS.items():          # wgrad: dW[Mout][Nin] += dY[R][Mout]^T X[R][Nin], splitk = splitk_for(Mout, Nin, R)
        add(f"C_wgrad_{Mo}x{Ni}x{R}_splitk{sk}", "C", Mo, Ni, R, "tn", 2300 + sk, accumulate=2, splitk=sk)
    # D. batch: the production call patterns (tacotron2_amd/engine.py), Bt = 3, L = 37, T = 19, Ad = 24
    Bt, L, T, Ad = 3, 37, 19, 24
    for Ef in (40, 42):
        s = 3000 + Ef
        # (a) pmT[b] = W_att x memory[b]^T: A broadcast
        add(f"D_a_broadcastA_Ef{Ef}", "D", Ad, L, Ef, "nt", s, batch=Bt, lda=Ef, ldb=Ef, sA=0, sB=L * Ef)
        # (b) dmem[b] = align[b]^T x dctx_tot[:, b]: the batch interleaved in B's rows
        add(f"D_b_interleavedB_Ef{Ef}", "D", L, Ef, T, "tn", s + 100, batch=Bt, lda=L, ldb=Bt * Ef, sA=T * L, sB=Ef)
        # (c) dmem[b] += dpmT[b]^T x W_att: B broadcast, plain accumulate
        add(f"D_c_broadcastB_acc1_Ef{Ef}", "D", L, Ef, Ad, "tn", s + 200, batch=Bt, lda=L, ldb=Ef, sA=Ad * L, sB=0, accumulate=1)
        # (d) dW_att += sum_b dpmT[b] x memory[b]: the batch reduced into one C through atomics
        add(f"D_d_reduce_Ef{Ef}", "D", Ad, Ef, L, "nn", s + 300, batch=Bt, lda=L, ldb=Ef, sA=Ad * L, sB=L * Ef, sC=0, accumulate=2)
        # (e) (a) with split-K
        add(f"D_e_broadcastA_splitk2_Ef{Ef}", "D", Ad, L, Ef, "nt", s + 400, batch=Bt, lda=Ef, ldb=Ef, sA=0, sB=L * Ef, splitk=2,
            accumulate=2)
    # (a) with ld and base aligned and the batch stride alone off 4: only sB % 4 takes the vector loads away
    add("D_a_stride_off4", "D", Ad, L, 40, "nt", 3900, batch=Bt, lda=40, ldb=40, sA=0, sB=L * 40 + 2)
    # E. epilogue order
    e = dict(M=133, N=131, K=40, layout="nt")
    add("E_alpha_bias", "E", seed=4000, alpha=-0.75, bias=1, **e)
    add("E_acc1_relu_mask", "E", seed=4001, accumulate=1, relu=1, ldmask=131 + 5, bias=1, **e)
    add("E_relu_negative_alpha", "E", seed=4002, alpha=-0.75, relu=1, bias=1, **e)
    add("E_bias2_alone", "E", seed=4003, bias2=1, **e)
    add("E_dense_ldc", "E", seed=4004, ldc=131, bias=1, bias2=1, **e)
    # F. addressing features
    Ci = 16      # k = 5 'same' Conv1d over 3 padded samples of 21 + 4 rows: row m of A is the 5 * Ci elements from m * Ci on
    add("F_overlapping_rows", "F", 3 * (21 + 4) - 4, 24, 5 * Ci, "nt", 5000, lda=Ci, overlap=1, bias=1)
    # k = 3, dilation 3 on L = 137 rows of 32 channels: tap block j of row m = the 32 channels of row m + 3 j
    tap = dict(M=137, N=40, K=3 * 32, layout="nt", lda=32, a_tap_len=32, a_tap_stride=3 * 32, overlap=1, bias=1)
    add("F_tap_strided", "F", seed=5001, **tap)
    add("F_tap_strided_batch2", "F", seed=5002, batch=2, sA=(137 + 6) * 32, sB=0, **tap)
    return {c["name"]: c for c in cs}


# G. calls t2_gemm must refuse (T2_ERR_ARG, before any launch): (name, fields changed on VALID_CALL, words of the message).
# "ptr" stands for any non-NULL pointer.
VALID_CALL = dict(M=64, N=64, K=64, lda=64, ldb=64, ldc=64, a_kmajor=1, b_kmajor=1, alpha=1.0)
REJECTIONS = [
    ("splitk_without_atomics", dict(splitk=2, accumulate=0), "splitk>1 requires accumulate=2"),
    ("atomics_with_relu", dict(accumulate=2, relu=1), "atomic epilogue"),
    ("atomics_with_mask", dict(accumulate=2, mulmask="ptr", ldmask=64), "atomic epilogue"),
    ("a_mmajor_b_kmajor", dict(a_kmajor=0, b_kmajor=1), "layout not instantiated"),
    ("tap_len_24", dict(a_tap_len=24, a_tap_stride=24, K=72, lda=24), "a_tap_len"),
    ("tap_len_with_mmajor_a", dict(a_tap_len=32, a_tap_stride=32, a_kmajor=0, b_kmajor=0), "a_tap_len"),
    ("tap_len_32_k80", dict(a_tap_len=32, a_tap_stride=32, K=80, lda=32), "a_tap_len"),
    ("precision_3", dict(precision=3), "precision"),
    ("m_zero", dict(M=0), "empty dims"),
    ("null_a", dict(A=None), "null operand"),
    ("stat_out_native", dict(stat_out="ptr", stat_Lp=64, stat_L=60, native_fp32=1), "stat_out"),
    ("stat_out_batch", dict(stat_out="ptr", stat_Lp=64, stat_L=60, batch=2, sA=4096, sB=4096, sC=4096), "stat_out"),
    ("stat_out_splitk", dict(stat_out="ptr", stat_Lp=64, stat_L=60, splitk=2, accumulate=2), "stat_out"),
]

def rejected_call(make, overrides, A, B, C, extra):
    """The T2Gemm of VALID_CALL with `overrides` (make = tacotron2_amd._lib.make); "ptr" becomes `extra`."""
    kw = dict(VALID_CALL, A=A, B=B, C=C)
    kw.update({k: (extra if v == "ptr" else v) for k, v in overrides.items()})
    return make("T2Gemm", **kw)


TILE_MAPS = [(1, 1), (3, 1), (1, 3), (8, 1), (9, 1), (9, 3), (11, 2), (16, 2), (17, 1), (19, 3)]
K_EDGES = [1, 3, 4, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65]
PLACEMENTS = ("vec", "exact", "off1")
WGRADS = {(96, 160, 2100): 16, (512, 80, 900): 7}      # (Mout, Nin, R): engine.splitk_for(Mout, Nin, R) (asserted by the host test)
CASES = _cases()
