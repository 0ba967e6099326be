"""The host statement of UNetLoss under the focal and the soft Dice cost, which tests/test_unet_cost_gpu.py compares
`msau_unet_cost` / `msau_unet_cost_eval` against and tests/test_unet_cost_cpu.py pins to float64 torch autograd: plain float64 numpy,
a document at a time, under the rule of tests/kv_eval_util.py::unet_eval_host -- a pixel is active inside its document's extent with
a label in [0, C); every document computes what it computes alone; a head's loss is (1/B) sum_b L_b; the total is
0.5 final + 0.5 aux with two heads, else the final head."""
import numpy as np

FOCAL, DICE = "focal", "dice"


def focal_factor_host(pt, nll, gamma):
    """-> (f, m) per pixel: loss term f * nll, gradient m * (p - onehot).  gamma = 0: the cross entropy; where 1 - pt is 0 (and
    gamma > 0) both are 0"""
    pt, nll = np.asarray(pt, dtype=np.float64), np.asarray(nll, dtype=np.float64)
    if gamma == 0:
        return np.ones_like(pt), np.ones_like(pt)
    q = 1.0 - pt
    ok = q > 0
    qs = np.where(ok, q, 1.0)
    f = np.where(ok, qs ** gamma, 0.0)
    m = np.where(ok, f + gamma * pt * qs ** (gamma - 1.0) * nll, 0.0)
    return f, m


def dice_coef_host(I, P, Y, eps, v):
    """per class of one document -> (loss, hit, miss); v the class weights [C]"""
    V = v.sum()
    if not V > 0:
        return 0.0, np.zeros_like(I), np.zeros_like(I)
    den = P + Y + eps
    miss = (v / V) * (2 * I + eps) / den ** 2
    hit = miss - (v / V) * 2 / den
    return 1.0 - float(((v / V) * (2 * I + eps) / den).sum()), hit, miss


def unet_cost_host(kind, param, logits, aux, labels, aux_labels, sizes=None, cw=None):
    """kind "focal" (param = gamma >= 0) or "dice" (param = smooth > 0); logits / aux: [B, H, W, >= C] arrays (aux None: one head),
    only the first C channels are read, C = len(cw) if given else the channel count; labels / aux_labels int [B, H, W]; sizes
    [B][2] = (h, w) or None (dense).  -> (loss3 float64 [3] = (total, final, aux), doc_loss float64 [B, 2], grads: per head float64
    [B, H, W, C], the gradient of the TOTAL, zero at every inactive pixel).  The absent head's entries are 0."""
    assert kind in (FOCAL, DICE)
    logits = np.asarray(logits, dtype=np.float64)
    B, H, W = logits.shape[:3]
    C = len(cw) if cw is not None else logits.shape[3]
    v = np.asarray(cw, dtype=np.float64) if cw is not None else np.ones(C)
    heads = [(logits, np.asarray(labels))] + ([(np.asarray(aux, dtype=np.float64), np.asarray(aux_labels))] if aux is not None else [])
    hwt = 0.5 if len(heads) == 2 else 1.0
    doc_loss, grads = np.zeros((B, 2)), []
    for t, (lg, lab) in enumerate(heads):
        g = np.zeros((B, H, W, C))
        for b in range(B):
            h, w = (int(sizes[b][0]), int(sizes[b][1])) if sizes is not None else (H, W)
            x = lg[b, :h, :w, :C].reshape(-1, C)
            tg = lab[b, :h, :w].reshape(-1).astype(np.int64)
            on = (tg >= 0) & (tg < C)
            if not on.any():
                continue
            x, tg = x[on], tg[on]
            n = len(tg)
            mx = x.max(axis=1, keepdims=True)
            lse = mx[:, 0] + np.log(np.exp(x - mx).sum(axis=1))
            p = np.exp(x - lse[:, None])
            onehot = np.zeros((n, C))
            onehot[np.arange(n), tg] = 1.0
            if kind == FOCAL:
                D = (h * w) if cw is None else v[tg].sum()
                if not D > 0:
                    continue
                nll = lse - x[np.arange(n), tg]
                f, m = focal_factor_host(p[np.arange(n), tg], nll, param)
                doc_loss[b, t] = (v[tg] * f * nll).sum() / D
                gd = (v[tg] * m / (B * D))[:, None] * (p - onehot)
            else:
                I, P, Y = (p * onehot).sum(axis=0), p.sum(axis=0), onehot.sum(axis=0)
                doc_loss[b, t], hit, miss = dice_coef_host(I, P, Y, param, v)
                a = np.where(onehot > 0, hit[None, :], miss[None, :])
                gd = p * (a - (a * p).sum(axis=1, keepdims=True)) / B
            full = np.zeros((h * w, C))
            full[on] = hwt * gd
            g[b, :h, :w] = full.reshape(h, w, C)
        grads.append(g)
    final, auxl = doc_loss[:, 0].mean(), doc_loss[:, 1].mean()
    loss3 = np.array([0.5 * final + 0.5 * auxl if len(heads) == 2 else final, final, auxl])
    return loss3, doc_loss, grads
