"""Edit distance and error rates (reference utils/evaluation/edit_distance.py)
scored on the device (native_ops.edit_distance, csrc/edit_distance.hip).

compute_wer / compute_cer / compute_per keep the reference's signatures and
return contracts for any hashable items: the items are interned to integers,
uploaded and scored by the kernel.  compute_cer / compute_per return the
distance only, as the reference does, without its Levenshtein dependency.

Where the reference's backtrace has no rule -- on the table's borders its
indices wrap and it raises IndexError, e.g. for every empty hypothesis -- the
moves are insertions at x == 0 and deletions at y == 0.

ErrorRateMeter accumulates (distance, sub, ins, del, reference units) over an
evaluation in a device tensor: update() takes the decoders' device outputs as
they are and never synchronises; result() does the single host read.
"""
import numpy as np
import torch

from ... import native_ops as ops


def _device():
    return torch.device('cuda', torch.cuda.current_device())


def _score_pair(ref, hyp):
    ref, hyp = list(ref), list(hyp)
    ids = {}
    r = np.array([[ids.setdefault(u, len(ids)) for u in ref] or [-1]], np.int32)
    h = np.array([[ids.setdefault(u, len(ids)) for u in hyp] or [-1]], np.int32)
    dev = _device()
    out = ops.edit_distance(torch.from_numpy(h).to(dev), [len(hyp)], torch.from_numpy(r).to(dev),
                            [len(ref)])
    return [int(v) for v in out[0].cpu().numpy()]


def compute_wer(ref, hyp, normalize=False):
    """Word error rate of two word lists (any hashable items).
    Returns (wer, sub, ins, dele); wer is the distance, divided by len(ref) if
    normalize."""
    wer, sub, ins, dele, _ = _score_pair(ref, hyp)
    if normalize:
        wer /= len(ref)
    return wer, sub, ins, dele


def compute_cer(ref, hyp, normalize=False):
    """Character error rate of two strings (or item sequences): the distance,
    divided by len(ref) if normalize."""
    cer = _score_pair(ref, hyp)[0]
    if normalize:
        cer /= len(list(ref))
    return cer


def compute_per(ref, hyp, normalize=False):
    """Phone error rate of two phone lists: the distance, divided by len(ref)
    if normalize."""
    per = _score_pair(ref, hyp)[0]
    if normalize:
        per /= len(ref)
    return per


class ErrorRateMeter(object):
    """Running error counts of one evaluation, resident on the device.

    unit 'token' or 'word'; eos / space / token_map as native_ops.edit_distance
    (token_map: int sequence, token -> token or -1 to delete; uploaded once).
    """

    def __init__(self, unit, eos=None, space=None, token_map=None):
        if unit not in ('token', 'word'):
            raise ValueError("unit must be 'token' or 'word'")
        if unit == 'word' and space is None:
            raise ValueError("unit 'word' needs the separator token (space)")
        self.unit, self.eos, self.space = unit, eos, space
        self._map_host = None if token_map is None else np.asarray(token_map).astype(np.int32)
        self._map = {}
        self._totals = {}
        self.utterances = 0

    def update(self, hyp, hyp_lens, ref, ref_lens):
        """Scores one batch (device tensors; lengths may be host arrays) and
        adds it to the totals.  Returns the batch's int32 [B, 5] device tensor."""
        dev = hyp.device
        if dev not in self._totals:
            self._totals[dev] = torch.zeros(5, dtype=torch.int64, device=dev)
            if self._map_host is not None:
                self._map[dev] = torch.from_numpy(self._map_host).to(dev)
        out = ops.edit_distance(hyp, hyp_lens, ref, ref_lens, unit=self.unit, eos=self.eos,
                                space=self.space, token_map=self._map.get(dev),
                                totals=self._totals[dev])
        self.utterances += int(hyp.shape[0])
        return out

    def reset(self):
        self._totals = {}
        self.utterances = 0

    def result(self):
        """The evaluation's single host read."""
        t = np.zeros(5, np.int64)
        for v in self._totals.values():
            t += v.cpu().numpy()
        dist, sub, ins, dele, units = (int(v) for v in t)
        return dict(rate=dist / units if units else float('nan'), distance=dist, sub=sub, ins=ins,
                    dele=dele, ref_units=units, utterances=self.utterances)


def score_decoded(meter, device, hyp_d, hyp_lens_d, host_hyps, ys, y_lens, perm_idx):
    """The shared tail of the models' error_rate(): hypotheses that are still
    host arrays (host_hyps, ragged) are uploaded, ys / y_lens are reordered by
    the decode's perm_idx, and the batch goes through the meter."""
    if hyp_d is None:
        B = len(host_hyps)
        L = max([len(h) for h in host_hyps] + [1])
        buf = np.full((B, L), -1, np.int32)
        for b, h in enumerate(host_hyps):
            buf[b, :len(h)] = np.asarray(h)
        hyp_d = ops.h2d(buf, device)
        hyp_lens_d = ops.h2d(np.array([len(h) for h in host_hyps], np.int32), device)
    perm = np.asarray(perm_idx).reshape(-1)
    ys = np.asarray(ys)
    if ys.ndim != 2:
        raise ValueError('ys must be a padded [B, L] label array')
    ref_d = ops.h2d(ys[perm].astype(np.int32), device)
    ref_lens_d = ops.h2d(np.asarray(y_lens).reshape(-1)[perm].astype(np.int32), device)
    return meter.update(hyp_d, hyp_lens_d, ref_d, ref_lens_d)
