"""The host statement of the masked cost: the loss of `TrainEngine.step` / `MSAUWrapper.loss` with class weights and
under the focal and the soft Dice cost, which tests/test_masked_cost_gpu.py compares `msau_masked_cost` / `msau_masked_cost_eval`
against and tests/test_masked_cost_cpu.py pins to float64 torch autograd.  Plain float64 numpy, a document at a time, written from
the statement and not from the kernels: a pixel is active inside its document's extent with a label in [1, C); both heads are scored
against the same label map; every document computes what it computes alone; a head's loss is (1/B) sum_b L_b; the total is
final + aux."""
import numpy as np

from tests.unet_cost_util import DICE, FOCAL, dice_coef_host, focal_factor_host

CE = "cross_entropy"


def masked_cost_host(kind, param, logits, aux, labels, sizes=None, cw=None):
    """kind CE (param unread), FOCAL (param = gamma >= 0) or DICE (param = smooth > 0); logits / aux: [B, H, W, >= C] arrays (aux
    None: one head), only the first C channels are read, C = len(cw) if given else the channel count; labels int [B, H, W]; sizes
    [B][2] = (h, w) or None (dense).  -> (loss3 float64 [3] = (total, final, aux), doc_loss float64 [B, 2], grads: per head float64
    [B, H, W, C], the gradient of the TOTAL, zero at every inactive pixel).  The absent head's entries are 0."""
    assert kind in (CE, FOCAL, DICE)
    logits = np.asarray(logits, dtype=np.float64)
    labels = np.asarray(labels)
    B, H, W = logits.shape[:3]
    C = len(cw) if cw is not None else logits.shape[3]
    v = np.asarray(cw, dtype=np.float64) if cw is not None else np.ones(C)
    heads = [logits] + ([np.asarray(aux, dtype=np.float64)] if aux is not None else [])
    doc_loss, grads = np.zeros((B, 2)), []
    for t, lg in enumerate(heads):
        g = np.zeros((B, H, W, C))
        for b in range(B):
            h, w = (int(sizes[b][0]), int(sizes[b][1])) if sizes is not None else (H, W)
            x = lg[b, :h, :w, :C].reshape(-1, C)
            tg = labels[b, :h, :w].reshape(-1).astype(np.int64)
            on = (tg >= 1) & (tg < C)
            if not on.any():
                continue                                                     # no active pixel: loss 0, gradient 0
            x, tg = x[on], tg[on]
            n = len(tg)
            mx = x.max(axis=1, keepdims=True)
            lse = mx[:, 0] + np.log(np.exp(x - mx).sum(axis=1))
            p = np.exp(x - lse[:, None])
            onehot = np.zeros((n, C))
            onehot[np.arange(n), tg] = 1.0
            if kind == DICE:
                I, P, Y = (p * onehot).sum(axis=0), p.sum(axis=0), onehot.sum(axis=0)      # Y[0] = 0: no active pixel has label 0
                doc_loss[b, t], hit, miss = dice_coef_host(I, P, Y, param, v)
                a = np.where(onehot > 0, hit[None, :], miss[None, :])
                gd = p * (a - (a * p).sum(axis=1, keepdims=True)) / B
            else:
                D = v[tg].sum()
                if not D > 0:
                    continue
                nll = lse - x[np.arange(n), tg]
                f, m = focal_factor_host(p[np.arange(n), tg], nll, param if kind == FOCAL else 0.0)
                doc_loss[b, t] = (v[tg] * f * nll).sum() / D
                gd = (v[tg] * m / (B * D))[:, None] * (p - onehot)
            full = np.zeros((h * w, C))
            full[on] = gd
            g[b, :h, :w] = full.reshape(h, w, C)
        grads.append(g)
    final, auxl = doc_loss[:, 0].mean(), doc_loss[:, 1].mean()
    return np.array([final + auxl, final, auxl]), doc_loss, grads


def counts_host(logits, aux, labels, sizes=None, C=None):
    """-> int [B, 2, 2]: per document and head (labelled, correct) over the active pixels, the prediction the first maximum of the
    C real logits; zeros for an absent head"""
    labels = np.asarray(labels)
    B, H, W = labels.shape
    C = C or np.asarray(logits).shape[3]
    out = np.zeros((B, 2, 2), dtype=np.int64)
    for t, lg in enumerate([logits] + ([aux] if aux is not None else [])):
        lg = np.asarray(lg, dtype=np.float64)
        for b in range(B):
            h, w = (int(sizes[b][0]), int(sizes[b][1])) if sizes is not None else (H, W)
            tg = labels[b, :h, :w]
            on = (tg >= 1) & (tg < C)
            pred = lg[b, :h, :w, :C].argmax(axis=-1)
            out[b, t] = (int(on.sum()), int((pred[on] == tg[on]).sum()))
    return out
