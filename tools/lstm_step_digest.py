"""One sha256 per output tensor of fixed-seed cases through every LSTM step kernel of t2_lstm.hip (forward generic / packed /
square-tile / persistent, backward packed 4- and 8-wave / generic), through the C ABI only (_lib.make, _lib.call, and arrays of
the _lib.S structs where a call takes two descriptors), so that the
same file runs against two builds of the library (T2_LIB_PATH selects one) and their outputs can be compared bit for bit.

    python tools/lstm_step_digest.py [--save OUT.pt] [--against OTHER.pt]

--save keeps the output tensors; --against prints, for every tensor that differs from the saved ones of another build, the
maximum absolute difference."""
import argparse
import hashlib
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from tacotron2_amd import _lib  # noqa: E402

DEV = torch.device("cuda:0")
OUT = {}


def stream():
    return torch.cuda.current_stream().cuda_stream


def record(case, **tensors):
    torch.cuda.synchronize()
    for name, t in tensors.items():
        OUT[f"{case}.{name}"] = t.detach().cpu().contiguous()


def tile16(x, Bp):
    B, K = x.shape
    out = torch.zeros(K // 16, Bp, 16)
    out[:, :B] = x.reshape(B, K // 16, 16).permute(1, 0, 2)
    return out


def lens_of(B):
    return torch.tensor([3 if i % 4 == 1 else 9 for i in range(B)], dtype=torch.int32)


def pack_fwd(Ws, H):
    K = sum(W.shape[1] for W in Ws)
    segs = (_lib.S["T2Seg"] * len(Ws))()
    for i, W in enumerate(Ws):
        segs[i].w = W.data_ptr(); segs[i].ldw = W.shape[1]; segs[i].K = W.shape[1]
    wp = torch.empty(H // 4 * ((K // 16 + 15) // 16 * 16) * 256, device=DEV)
    _lib.call("t2_lstm_pack_fwd", segs, len(Ws), H, wp, stream())
    return wp


def fwd_cell_operands(g, B, H, keep):
    """One forward cell's epilogue operands and outputs (every optional one present)."""
    d = dict(pre=torch.randn(B, 4 * H, generator=g), bias1=torch.randn(4 * H, generator=g), bias2=torch.randn(4 * H, generator=g),
             c_prev=torch.randn(B, H, generator=g), drop=(torch.rand(B, H, generator=g) > 0.1).float() / 0.9)
    d = {k: v.to(DEV) for k, v in d.items()}
    d["len"] = lens_of(B).to(DEV)
    out = dict(h_out=torch.zeros(B, H, device=DEV), h_out2=torch.zeros(B, H + 8, device=DEV), c_out=torch.zeros(B, H, device=DEV),
               gates_out=torch.zeros(B, 4 * H, device=DEV))
    keep += list(d.values()) + list(out.values())
    kw = dict(B=B, H=H, ldpre=4 * H, ldc_prev=H, lddrop=H, ldh=H, ldh2=H + 8, ldc_out=H, ldg=4 * H, t=5, **d, **out)
    return kw, out


def fwd_generic(case, B, H, Ks, n):
    g = torch.Generator().manual_seed(1000 + B + H + n)
    steps = (_lib.S["T2LstmStep"] * 2)()
    keep, outs = [], []
    for i in range(n):
        kw, out = fwd_cell_operands(g, B, H, keep)
        st = _lib.make("T2LstmStep", nseg=len(Ks), **kw)
        for j, K in enumerate(Ks):
            x = torch.randn(B, K, generator=g).to(DEV); W = (torch.randn(4 * H, K, generator=g) / K ** 0.5).to(DEV)
            keep += [x, W]
            st.seg[j].x = x.data_ptr(); st.seg[j].ldx = K; st.seg[j].w = W.data_ptr(); st.seg[j].ldw = K; st.seg[j].K = K
        steps[i] = st
        outs.append(out)
    _lib.call("t2_lstm_step_fwd", steps, n, stream())
    for i, out in enumerate(outs):
        record(f"{case}.cell{i}", **out)


def fwd_packed(case, B, H, Ks, col0, tiled):
    g = torch.Generator().manual_seed(2000 + B * 7 + H)
    K = sum(Ks)
    keep = []
    kw, out = fwd_cell_operands(g, B, H, keep)
    x = torch.randn(B, K, generator=g)
    Ws = [(torch.randn(4 * H, k, generator=g) / K ** 0.5).to(DEV) for k in Ks]
    wp = pack_fwd(Ws, H)
    Bp = (B + 15) // 16 * 16
    xt = tile16(x, Bp).to(DEV); xd = x.to(DEV)
    ht = torch.full(((col0 + H + 15) // 16, Bp, 16), -7.0, device=DEV)
    st = _lib.make("T2LstmStep", nseg=1, wpacked=wp, xt=xt if tiled else None, ht_out=ht if tiled else None, ht_col0=col0, **kw)
    st.seg[0].x = xd.data_ptr(); st.seg[0].ldx = K; st.seg[0].K = K
    _lib.call("t2_lstm_step_fwd", st, 1, stream())
    record(case, ht=ht, **out)


def fwd_persistent(case, B, H, S):
    g = torch.Generator().manual_seed(3000 + B + H + S)
    Bp = (B + 15) // 16 * 16
    W = (torch.randn(4 * H, H, generator=g) / H ** 0.5).to(DEV)
    pre = torch.randn(S, B, 4 * H, generator=g).to(DEV)
    drop = ((torch.rand(S, B, H, generator=g) > 0.1).float() / 0.9).to(DEV)
    b1 = torch.randn(4 * H, generator=g).to(DEV); b2 = torch.randn(4 * H, generator=g).to(DEV)
    h0, c0 = torch.randn(B, H, generator=g) * 0.5, torch.randn(B, H, generator=g) * 0.5
    lens = torch.tensor([1 if i % 4 == 1 else 9 for i in range(B)], dtype=torch.int32).to(DEV)
    wp = pack_fwd([W], H)
    ht = torch.zeros(S + 1, H // 16, Bp, 16, device=DEV); ht[0] = tile16(h0, Bp).to(DEV)
    hrow = torch.zeros(S + 1, B, H, device=DEV); hrow[0] = h0.to(DEV)
    hrow2 = torch.zeros(S, B, H + 8, device=DEV)
    cs = torch.zeros(S + 1, B, H, device=DEV); cs[0] = c0.to(DEV)
    gs = torch.zeros(S, B, 4 * H, device=DEV)
    st = _lib.make("T2LstmStep", B=B, H=H, nseg=1, wpacked=wp, pre=pre, ldpre=4 * H, bias1=b1, bias2=b2, c_prev=cs, ldc_prev=H,
                   drop=drop, lddrop=H, h_out=hrow[1], ldh=H, h_out2=hrow2, ldh2=H + 8, c_out=cs[1], ldc_out=H, gates_out=gs,
                   ldg=4 * H, len=lens, t=0, xt=ht, ht_out=ht[1], ht_col0=0)
    st.seg[0].x = hrow.data_ptr(); st.seg[0].ldx = H; st.seg[0].w = W.data_ptr(); st.seg[0].ldw = H; st.seg[0].K = H
    inc = _lib.make("T2LstmStride", pre=B * 4 * H, c_prev=B * H, drop=B * H, h_out=B * H, h_out2=B * (H + 8), c_out=B * H,
                    gates_out=B * 4 * H, dt=1, xt=H * Bp, ht_out=H * Bp)
    inc.seg_x[0] = B * H
    sync = torch.zeros(320, dtype=torch.int32, device=DEV)
    _lib.call("t2_lstm_seq_fwd_persist", st, inc, S, sync, stream())
    torch.cuda.synchronize()
    assert int(sync[256]) == 0, "an inter-workgroup wait timed out"
    record(case, h=hrow, h2=hrow2, c=cs, gates=gs, ht=ht)


def bwd(case, B, H, N4, ncols, epi, packed, recurrent=True, tiled=False):
    g = torch.Generator().manual_seed(4000 + B + N4 + ncols + epi)
    W = (torch.randn(N4, ncols, generator=g) / N4 ** 0.5).to(DEV)
    dg = torch.randn(B, N4, generator=g)
    Bp = (B + 15) // 16 * 16
    dgt = tile16(dg, Bp).to(DEV); dg = dg.to(DEV)
    e1 = torch.randn(B, ncols, generator=g).to(DEV); e2 = torch.randn(B, ncols, generator=g).to(DEV)
    gates = (torch.rand(B, 4 * H, generator=g) * 0.8 + 0.1).to(DEV)
    cp = torch.randn(B, H, generator=g).to(DEV); cc = torch.randn(B, H, generator=g).to(DEV); dc = torch.randn(B, H, generator=g).to(DEV)
    drop = ((torch.rand(B, H, generator=g) > 0.1).float() / 0.9).to(DEV)
    lens = lens_of(B).to(DEV)
    wtp = None
    if packed:
        wtp = torch.empty((ncols + 15) // 16 * ((N4 // 16 + 31) // 32 * 32) * 256, device=DEV)
        _lib.call("t2_lstm_pack_bwd", W, ncols, N4, None, 0, 0, ncols, wtp, stream())
    dx = torch.zeros(B, ncols, device=DEV); dgo = torch.zeros(B, 4 * H, device=DEV); dgo2 = torch.zeros(B, 8 * H, device=DEV)
    dgo_t = torch.zeros(4 * H // 16, Bp, 16, device=DEV) if tiled else None
    st = _lib.make("T2LstmBwdStep", B=B, H=H, N4=N4, dg_next=dg if recurrent else None, lddg=N4, W=W, ldw=ncols, wtpacked=wtp,
                   ncols=ncols, epi=epi, ext1=e1, ldx1=ncols, ext2=e2, ldx2=ncols, dx_out=dx, lddx=ncols, drop=drop, lddrop=H,
                   gates=gates, ldgs=4 * H, c_prev=cp, ldcp=H, c_cur=cc, ldcc=H, dc=dc, lddc=H, dg_out=dgo, ldgo=4 * H,
                   dg_out2=dgo2, ldgo2=8 * H, len=lens, t=5, dgt_next=dgt if tiled else None, dgt_out=dgo_t)
    _lib.call("t2_lstm_step_bwd", st, 1, stream())
    if epi == 0:
        record(case, dx=dx)
    elif tiled:
        record(case, dg=dgo, dg2=dgo2, dc=dc, dgt=dgo_t)
    else:
        record(case, dg=dgo, dg2=dgo2, dc=dc)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--save")
    ap.add_argument("--against")
    args = ap.parse_args()
    # forward, generic kernel: 1 and 2 cells per launch, 1 to 3 segments (MT = 1, 2, 4)
    fwd_generic("fwd_generic.3x32.seg2", 3, 32, (16, 32), 1)
    fwd_generic("fwd_generic.17x64.seg3", 17, 64, (16, 32, 64), 1)
    fwd_generic("fwd_generic.64x256.seg1", 64, 256, (256,), 1)
    fwd_generic("fwd_generic.17x64.seg2.two_cells", 17, 64, (16, 32), 2)
    # forward, packed kernel: MT = 1, 2, 4 with row-major and tiled input; the square-tile kernel (tiled, 33..64 rows, H % 64 == 0)
    for tiled in (False, True):
        tag = "tiled" if tiled else "rows"
        fwd_packed(f"fwd_packed.mt1.5x64.{tag}", 5, 64, (48,), 16, tiled)
        fwd_packed(f"fwd_packed.mt2.19x32.{tag}", 19, 32, (32,), 32, tiled)
        fwd_packed(f"fwd_packed.mt4.40x32.{tag}", 40, 32, (32,), 0, tiled)
    fwd_packed("fwd_packed.mt4.64x128.rows", 64, 128, (128, 64), 0, False)
    fwd_packed("fwd_square.64x128", 64, 128, (128, 64), 0, True)
    fwd_packed("fwd_square.35x64", 35, 64, (64,), 0, True)
    fwd_persistent("fwd_persistent.5x64.s4", 5, 64, 4)
    fwd_persistent("fwd_persistent.35x128.s3", 35, 128, 3)
    # backward, packed: 8 waves up to 64 workgroups, 4 waves above; plain products (epi 0) and the cell backward (epi 1)
    bwd("bwd_packed8.epi1.7x48", 7, 48, 192, 48, 1, True, tiled=True)
    bwd("bwd_packed8.epi1.33x64", 33, 64, 256, 64, 1, True)
    bwd("bwd_packed8.epi0.33x40", 33, 64, 256, 40, 0, True)
    bwd("bwd_packed4.epi1.17x528", 17, 528, 64, 528, 1, True, tiled=True)
    bwd("bwd_packed4.epi0.17x520", 17, 528, 64, 520, 0, True)
    # backward, generic kernel (the one whose sum order changes): with and without the recurrent product
    bwd("bwd_generic.epi1.19x48", 19, 48, 192, 48, 1, False)
    bwd("bwd_generic.epi1.19x48.no_dg_next", 19, 48, 192, 48, 1, False, recurrent=False)
    bwd("bwd_generic.epi0.19x40", 19, 48, 192, 40, 0, False)
    other = torch.load(args.against) if args.against else None
    for name, t in OUT.items():
        line = f"{hashlib.sha256(t.numpy().tobytes()).hexdigest()}  {name}  {tuple(t.shape)}"
        if other is not None and not torch.equal(other[name], t):
            line += f"  DIFFERS: max abs difference {float((other[name].double() - t.double()).abs().max()):.3e}"
        print(line)
    if other is not None:
        print("# tensors that differ from", os.path.basename(args.against), ":",
              [n for n, t in OUT.items() if not torch.equal(other[n], t)] or "none")
    if args.save:
        torch.save(OUT, args.save)


if __name__ == "__main__":
    main()
