#!/usr/bin/env python3
"""The bits of csrc/loss.hip: every entry point of the loss family on seeded inputs, one line per (call, case) with a sha256 over the
call's output buffers.  Two libraries compute the same bits when their outputs are equal line for line:

    MSAU_HIP_LIB=/path/to/parent/libmsau_hip.so python tools/loss_bits.py > parent.txt
    python tools/loss_bits.py > new.txt && diff parent.txt new.txt

(one fresh process per library).  B = 3 documents on a 37 x 29 canvas, fp32 and bf16; labels in [-1, C]; document 1 has no labelled
pixel (all 0; all -1 in the auxiliary label map); one class weight is 0; random values in the padded channels."""
import hashlib
import itertools
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from msau_amd import _lib as L

B, H, W = 3, 37, 29
EXTENTS = [(37, 29), (8, 6), (1, 1)]
PAIRS = [(5, 8), (8, 8), (13, 16), (17, 24), (26, 32), (32, 32), (40, 40), (17, 40), (5, 40)]          # (C, Cs)
COSTS = [(L.COST_CE, 0.0), (L.COST_FOCAL, 0.5), (L.COST_FOCAL, 2.0), (L.COST_DICE, 1.0), (L.COST_DICE, 1e-3)]
EVAL_KS = (1, 4, 7)
HIST_K = 4
DEV = None


def digest(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        t = t.detach().cpu().contiguous()
        h.update(t.view(torch.uint8).numpy().tobytes() if t.numel() else b"")
    return h.hexdigest()


def emit(call, case, *tensors):
    torch.cuda.synchronize()
    print(call, " ".join(f"{k}={v}" for k, v in case.items()), digest(*tensors), flush=True)


def stream():
    return torch.cuda.current_stream().cuda_stream


def ptr(t):
    return t.data_ptr() if t is not None else None


def inputs(C, Cs, dtype):
    td = torch.float32 if dtype == "fp32" else torch.bfloat16
    g = torch.Generator().manual_seed(100 * C + Cs)
    lg = [(torch.randn(B, H, W, Cs, generator=g) * 2).to(td).to(DEV) for _ in range(2)]
    labs = [torch.randint(-1, C + 1, (B, H, W), generator=g) for _ in range(2)]
    labs[0][1], labs[1][1] = 0, -1
    cw = torch.rand(C, generator=g) + 0.5
    cw[2] = 0.0
    return lg, [x.to(DEV) for x in labs], cw.to(DEV), torch.tensor(EXTENTS, dtype=torch.int32, device=DEV)


def fresh(like, n=1):
    return [torch.full_like(like, 9.0) for _ in range(n)]


def labels_only(lib):
    for C in sorted({c for c, _ in PAIRS}):
        _lg, labs, _cw, ext = inputs(C, 8 * -(-C // 8), "fp32")
        counts, split = torch.full((B,), 77, dtype=torch.int32, device=DEV), torch.full((B, 4), 77, dtype=torch.int32, device=DEV)
        L.call("msau_label_counts", stream(), labs[0].data_ptr(), counts.data_ptr(), B, H * W)
        emit("msau_label_counts", {"C": C}, counts)
        L.call("msau_label_counts_split", stream(), labs[0].data_ptr(), split.data_ptr(), B, H * W, 4)
        emit("msau_label_counts_split", {"C": C, "K": 4}, split)
        for e in (None, ext):
            hist = torch.full((B, HIST_K, C), 77, dtype=torch.int32, device=DEV)
            L.call("msau_label_hist", stream(), labs[0].data_ptr(), ptr(e), hist.data_ptr(), B, H, W, C, HIST_K)
            emit("msau_label_hist", {"C": C, "K": HIST_K, "ragged": e is not None}, hist)


def one_head(lib, C, Cs, dtype):
    dt = L.F32 if dtype == "fp32" else L.BF16
    lg, labs, cw, _ext = inputs(C, Cs, dtype)
    case = {"C": C, "Cs": Cs, "dtype": dtype}
    counts, split = torch.zeros(B, dtype=torch.int32, device=DEV), torch.zeros((B, 4), dtype=torch.int32, device=DEV)
    L.call("msau_label_counts", stream(), labs[0].data_ptr(), counts.data_ptr(), B, H * W)
    L.call("msau_label_counts_split", stream(), labs[0].data_ptr(), split.data_ptr(), B, H * W, 4)
    ws = torch.zeros(int(max(lib.msau_ce_ws_floats(B * H * W), lib.msau_ce_multi_ws_floats(B * H * W))), device=DEV)
    (d,), loss = fresh(lg[0]), torch.zeros(2, device=DEV)
    L.call("msau_masked_ce", stream(), dt, lg[0].data_ptr(), labs[0].data_ptr(), counts.data_ptr(), d.data_ptr(), loss.data_ptr(), ws.data_ptr(),
           B, H * W, C, Cs, 1.0 / B)
    emit("msau_masked_ce", case, loss, d)
    (d,), loss = fresh(lg[0]), torch.zeros(2, device=DEV)
    L.call("msau_softmax_ce", stream(), dt, lg[0].data_ptr(), labs[0].data_ptr(), d.data_ptr(), loss.data_ptr(), ws.data_ptr(), B, H * W, C, Cs,
           1.0 / (B * H * W))
    emit("msau_softmax_ce", case, loss, d)
    (d,), loss = fresh(lg[0]), torch.zeros(2, device=DEV)
    L.call("msau_softmax_ce_weighted", stream(), dt, lg[0].data_ptr(), labs[0].data_ptr(), cw.data_ptr(), d.data_ptr(), loss.data_ptr(),
           ws.data_ptr(), B, H * W, C, Cs)
    emit("msau_softmax_ce_weighted", case, loss, d)
    if Cs > 16:
        return
    for aux, k in itertools.product((False, True), (1, 4)):
        d, loss = fresh(lg[0], 2), torch.zeros(2, device=DEV)
        L.call("msau_masked_ce_multi", stream(), dt, lg[0].data_ptr(), lg[1].data_ptr() if aux else None, labs[0].data_ptr(),
               (counts if k == 1 else split).data_ptr(), d[0].data_ptr(), d[1].data_ptr() if aux else None, loss.data_ptr(), ws.data_ptr(),
               B, H * W, C, Cs, 1.0 / B, k)
        emit("msau_masked_ce_multi", dict(case, aux=aux, counts_k=k), loss, *d)


def two_heads(lib, C, Cs, dtype):
    dt = L.F32 if dtype == "fp32" else L.BF16
    lg, labs, cw, ext = inputs(C, Cs, dtype)
    dims = (B, H, W, C, Cs)
    for e in (None, ext):
        hist = torch.zeros((2, B, HIST_K, C), dtype=torch.int32, device=DEV)
        for t in range(2):
            L.call("msau_label_hist", stream(), labs[t].data_ptr(), ptr(e), hist[t].data_ptr(), B, H, W, C, HIST_K)
        for aux, weighted in itertools.product((False, True), (False, True)):
            case = {"C": C, "Cs": Cs, "dtype": dtype, "ragged": e is not None, "aux": aux, "weights": weighted}
            heads = (lg[0].data_ptr(), lg[1].data_ptr() if aux else None, labs[0].data_ptr(), labs[1].data_ptr() if aux else None, ptr(e),
                     cw.data_ptr() if weighted else None)
            masked = (lg[0].data_ptr(), lg[1].data_ptr() if aux else None, labs[0].data_ptr(), ptr(e), cw.data_ptr() if weighted else None)
            # training
            d, loss3 = fresh(lg[0], 2), torch.full((3,), 123.0, device=DEV)
            ws = torch.zeros(int(lib.msau_unet_ce_ws_floats(B * H * W)), device=DEV)
            L.call("msau_unet_ce", stream(), dt, *heads, hist.data_ptr() if weighted else None, HIST_K, d[0].data_ptr(),
                   d[1].data_ptr() if aux else None, loss3.data_ptr(), ws.data_ptr(), *dims)
            emit("msau_unet_ce", case, loss3, *d)
            for kind, param in COSTS:
                need = weighted or kind == L.COST_DICE
                d, loss3 = fresh(lg[0], 2), torch.full((3,), 123.0, device=DEV)
                ws = torch.zeros(int(lib.msau_unet_cost_ws_floats(kind, B, H, W, C)), device=DEV)
                L.call("msau_unet_cost", stream(), dt, kind, param, *heads, hist.data_ptr() if need else None, HIST_K, d[0].data_ptr(),
                       d[1].data_ptr() if aux else None, loss3.data_ptr(), ws.data_ptr(), *dims)
                emit("msau_unet_cost", dict(case, kind=kind, param=param), loss3, *d)
                for own in ((False,) if need else (False, True)):               # own: the call takes the histogram itself
                    d, loss3 = fresh(lg[0], 2), torch.full((3,), 123.0, device=DEV)
                    ws = torch.zeros(int(lib.msau_masked_cost_ws_floats(kind, B, H, W, C)), device=DEV)
                    L.call("msau_masked_cost", stream(), dt, kind, param, *masked, None if own else hist[0].data_ptr(), HIST_K, d[0].data_ptr(),
                           d[1].data_ptr() if aux else None, loss3.data_ptr(), ws.data_ptr(), *dims)
                    emit("msau_masked_cost", dict(case, kind=kind, param=param, own_hist=own), loss3, *d)
            # evaluation
            for K in EVAL_KS:
                rows, cnt = torch.full((B, 2), 123.0, device=DEV), torch.full((B, 2, 2), 77, dtype=torch.int32, device=DEV)
                ws = torch.zeros(int(lib.msau_unet_eval_ws_bytes(B, K)), dtype=torch.uint8, device=DEV)
                L.call("msau_unet_eval", stream(), dt, *heads, K, rows.data_ptr(), cnt.data_ptr(), ws.data_ptr(), *dims)
                emit("msau_unet_eval", dict(case, K=K), rows, cnt)
                for kind, param in COSTS:
                    rows, cnt = torch.full((B, 2), 123.0, device=DEV), torch.full((B, 2, 2), 77, dtype=torch.int32, device=DEV)
                    ws = torch.zeros(int(lib.msau_unet_cost_eval_ws_bytes(kind, B, K, C)), dtype=torch.uint8, device=DEV)
                    L.call("msau_unet_cost_eval", stream(), dt, kind, param, *heads, K, rows.data_ptr(), cnt.data_ptr(), ws.data_ptr(), *dims)
                    emit("msau_unet_cost_eval", dict(case, K=K, kind=kind, param=param), rows, cnt)
                    rows, cnt = torch.full((B, 2), 123.0, device=DEV), torch.full((B, 2, 2), 77, dtype=torch.int32, device=DEV)
                    ws = torch.zeros(int(lib.msau_masked_cost_eval_ws_bytes(kind, B, K, C)), dtype=torch.uint8, device=DEV)
                    L.call("msau_masked_cost_eval", stream(), dt, kind, param, *masked, K, rows.data_ptr(), cnt.data_ptr(), ws.data_ptr(), *dims)
                    emit("msau_masked_cost_eval", dict(case, K=K, kind=kind, param=param), rows, cnt)
        for zero_as in (-1, 1):
            counts = torch.zeros((C, C), dtype=torch.int64, device=DEV)
            L.call("msau_eval_confusion", stream(), dt, lg[0].data_ptr(), labs[0].data_ptr(), counts.data_ptr(), B, H, W, C, Cs, zero_as, ptr(e))
            emit("msau_eval_confusion", {"C": C, "Cs": Cs, "dtype": dtype, "ragged": e is not None, "zero_as": zero_as}, counts)


def softmax_heads(lib):
    for C in (5, 17):
        Cs = 8 * -(-C // 8)
        g = torch.Generator().manual_seed(C)
        x = (torch.randn(B, C, H, W, generator=g) * 2).to(DEV)
        pred = torch.full_like(x, 9.0)
        L.call("msau_softmax_channels_nchw", stream(), x.data_ptr(), pred.data_ptr(), B, C, H * W)
        emit("msau_softmax_channels_nchw", {"C": C}, pred)
        for dtype in ("fp32", "bf16"):
            lg = inputs(C, Cs, dtype)[0][0]
            probs, amax = torch.full((B, H, W, C), 9.0, device=DEV), torch.full((B, H, W), 77, dtype=torch.uint8, device=DEV)
            L.call("msau_softmax_argmax_nhwc", stream(), L.F32 if dtype == "fp32" else L.BF16, lg.data_ptr(), probs.data_ptr(), amax.data_ptr(),
                   B * H * W, C, Cs)
            emit("msau_softmax_argmax_nhwc", {"C": C, "Cs": Cs, "dtype": dtype}, probs, amax)


def main():
    global DEV
    if not torch.cuda.is_available():
        sys.exit("loss_bits.py runs the kernels: no GPU found")
    DEV = torch.device("cuda", 0)
    lib = L.load()
    labels_only(lib)
    for (C, Cs), dtype in itertools.product(PAIRS, ("fp32", "bf16")):
        one_head(lib, C, Cs, dtype)
        two_heads(lib, C, Cs, dtype)
    softmax_heads(lib)


if __name__ == "__main__":
    main()
