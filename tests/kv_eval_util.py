"""The host statement that tests/test_kv_eval_gpu.py compares `msau_unet_eval` against, pinned to msau_amd/training/cost.py::UNetLoss
(and through tests/golden/train/unet_loss*.npz to the reference) by tests/test_kv_eval_cpu.py: plain float64 numpy, a document at a
time."""
import numpy as np


def unet_eval_host(logits, aux, labels, aux_labels, sizes=None, cw=None):
    """logits / aux: [B, H, W, >= C] arrays (aux None: one head), only the first C channels are read, C = len(cw) if given else the
    channel count; labels / aux_labels int [B, H, W]; sizes [B][2] = (h, w) or None (dense).  -> (doc_loss float64 [B, 2],
    doc_counts int64 [B, 2, 2], near int64 [B, 2]):
      doc_loss[b][t]   = sum_p cw[t_p] nll_p / sum_p cw[t_p] over the pixels inside the extent with t_p in [0, C); 0 when the sum is 0
      doc_counts[b][t] = (pixels inside the extent with t_p in [1, C), those whose FIRST maximum is t_p)
      near[b][t]       = labelled pixels whose two largest logits are closer than 1e-4 (a rounding may decide their argmax)
    The absent head's rows are 0."""
    logits = np.asarray(logits, dtype=np.float64)
    B, H, W = logits.shape[:3]
    C = len(cw) if cw is not None else logits.shape[3]
    w_c = np.asarray(cw, dtype=np.float64) if cw is not None else np.ones(C)
    doc_loss, doc_counts, near = np.zeros((B, 2)), np.zeros((B, 2, 2), dtype=np.int64), np.zeros((B, 2), dtype=np.int64)
    heads = [(logits, np.asarray(labels))] + ([(np.asarray(aux, dtype=np.float64), np.asarray(aux_labels))] if aux is not None else [])
    for t, (lg, lab) in enumerate(heads):
        for b in range(B):
            h, w = (int(sizes[b][0]), int(sizes[b][1])) if sizes is not None else (H, W)
            x = lg[b, :h, :w, :C].reshape(-1, C)
            tg = lab[b, :h, :w].reshape(-1).astype(np.int64)
            on = (tg >= 0) & (tg < C)
            x, tg = x[on], tg[on]
            if len(tg) == 0:
                continue
            mx = x.max(axis=1, keepdims=True)
            lse = mx[:, 0] + np.log(np.exp(x - mx).sum(axis=1))
            nll = lse - x[np.arange(len(tg)), tg]
            wt = w_c[tg]
            den = wt.sum()
            if den > 0:
                doc_loss[b, t] = (wt[wt != 0] * nll[wt != 0]).sum() / den
            nz = tg >= 1
            pred = x.argmax(axis=1)                                        # numpy: the first maximum
            doc_counts[b, t] = (int(nz.sum()), int((pred[nz] == tg[nz]).sum()))
            if C >= 2:
                top = np.sort(x[nz], axis=1)[:, -2:]
                near[b, t] = int(((top[:, 1] - top[:, 0]) < 1e-4).sum())
    return doc_loss, doc_counts, near


def summary_host(doc_loss, doc_counts, has_aux=True):
    """(acc, loss, final) of a batch-1 epoch as the reference adds them up: means over documents"""
    final, aux = doc_loss[:, 0], doc_loss[:, 1]
    seen = doc_counts[:, 0, 0] > 0
    acc = float(np.mean(doc_counts[seen, 0, 1] / doc_counts[seen, 0, 0])) if seen.any() else float("nan")
    return acc, float(np.mean(0.5 * final + 0.5 * aux if has_aux else final)), float(np.mean(final))
