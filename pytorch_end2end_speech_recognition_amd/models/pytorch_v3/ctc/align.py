"""CTC forced alignment glue shared by CTC.align and
AttentionSeq2seq.align_ctc: the label checks that run before the encoder, and
the device search (native_ops.ctc_align) with its single host read."""
import numpy as np
import torch

from .... import native_ops as ops


def check_align_labels(ys, y_lens, num_labels):
    """ys padded [B, L] in the index space decode() returns (labels from 0),
    y_lens [B].  ValueError for a negative length, a length beyond ys' width,
    or a label outside [0, num_labels) among the first y_lens[b] of a row.
    Returns (ys int32, y_lens int32)."""
    ys = np.asarray(ys)
    if ys.ndim != 2:
        raise ValueError('align: ys must be a padded [B, L] label array')
    y_lens = np.asarray(y_lens).reshape(-1).astype(np.int64)
    if len(y_lens) != ys.shape[0]:
        raise ValueError('align: %d label lengths for %d rows' % (len(y_lens), ys.shape[0]))
    if (y_lens < 0).any():
        raise ValueError('align: negative label length')
    if (y_lens > ys.shape[1]).any():
        raise ValueError('align: a label length exceeds the width of ys (%d)' % ys.shape[1])
    used = ys[np.arange(ys.shape[1])[None, :] < y_lens[:, None]]
    if used.size and (used.min() < 0 or used.max() >= num_labels):
        raise ValueError('align: label outside [0, %d)' % num_labels)
    return ys.astype(np.int32), y_lens.astype(np.int32)


@torch.no_grad()
def align_logits(logits, lens_d, ys, y_lens, perm):
    """The alignment of ys[perm] (checked by check_align_labels) to `logits`
    [B, T, V] (blank 0, label c of ys = class c + 1).  Returns (alignments,
    spans, scores): alignments[b] int32 [out_len_b] in decode()'s index space
    with blank = -1, spans[b] int32 [L_b, 2] (first, last frame), scores
    float32 [B]; an infeasible row: an empty alignment, [0, 2] spans, -inf.
    One host read, after the search."""
    perm = np.asarray(perm).reshape(-1)
    ys, y_lens = ys[perm], y_lens[perm]
    B, L = ys.shape
    dev = logits.device
    flat = ys[np.arange(L)[None, :] < y_lens[:, None]].astype(np.int32) + 1
    lens = lens_d.to(dev).int().reshape(-1)
    ali, starts, ends, scores = ops.ctc_align(
        logits, lens, ops.h2d(flat, dev), ops.h2d(y_lens, dev), L, blank=0, normalize=True)
    T = ali.shape[1]
    packed = torch.cat([ali, starts, ends, scores.view(torch.int32).unsqueeze(1),
                        lens.unsqueeze(1)], dim=1).cpu().numpy()
    sc = np.ascontiguousarray(packed[:, T + 2 * L]).view(np.float32).copy()
    out_lens = packed[:, T + 2 * L + 1]
    alignments, spans = [], []
    for b in range(B):
        ok = sc[b] > -np.inf
        n = max(min(int(out_lens[b]), T), 0) if ok else 0
        k = int(y_lens[b]) if ok else 0
        alignments.append((packed[b, :n] - 1).astype(np.int32))
        spans.append(np.stack([packed[b, T:T + k], packed[b, T + L:T + L + k]], axis=1)
                     .astype(np.int32).reshape(k, 2))
    return (np.array(alignments + [None], dtype=object)[:-1],
            np.array(spans + [None], dtype=object)[:-1], sc)
