"""CTC prefix beam search decoder (reference beam_search_decoder.py:22-124).

The reference walks T x V x beam in Python; here the search runs on the
device (native_ops.ctc_beam_search, csrc/ctc_beam.hip) and only the compact
hypotheses cross PCIe.  numpy inputs (decode_from_probs) are uploaded to the
current device first: there is no host implementation.  Returns an object
array of int arrays (ragged; the reference's ``np.array(best_hyps)`` of ragged
lists fails on numpy >= 1.24).
"""
import numpy as np
import torch

from ..... import native_ops as ops


class BeamSearchDecoder(object):
    """Args as the reference: blank_index, space_index (unused there too)."""

    def __init__(self, blank_index, space_index=-1):
        self._blank = blank_index
        self._space = space_index

    def __call__(self, log_probs, x_lens, beam_width=1, alpha=0., beta=0., normalize=False):
        """log_probs [B, T, num_classes] (numpy or device tensor), x_lens [B].
        normalize=True: ``log_probs`` holds raw logits and the log-softmax is
        fused into the kernel.  alpha / beta (LM weight, insertion bonus) have
        no effect in the reference (no LM hook) and must be 0 here."""
        if alpha != 0 or beta != 0:
            raise NotImplementedError('BeamSearchDecoder: alpha / beta need a language model; '
                                      'the reference has no LM hook either')
        if not torch.is_tensor(log_probs):
            log_probs = torch.from_numpy(np.ascontiguousarray(log_probs, dtype=np.float32))
        if not log_probs.is_cuda:
            log_probs = log_probs.to(torch.device('cuda', torch.cuda.current_device()))
        if not torch.is_tensor(x_lens):
            x_lens = torch.as_tensor(np.asarray(x_lens).astype(np.int32))
        lens = x_lens.to(log_probs.device).int()
        hyps, hl, _ = ops.ctc_beam_search(log_probs, lens, int(beam_width), self._blank,
                                          normalize=normalize)
        hyps, hl = hyps.cpu().numpy(), hl.cpu().numpy()
        out = np.empty(len(hl), dtype=object)
        for b in range(len(hl)):
            out[b] = hyps[b, :hl[b]].astype(np.int64)
        return out
