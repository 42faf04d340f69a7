"""CTC model (reference models/pytorch_v3/ctc/ctc.py) on the MI355X hot path.

Drop-in: same constructor kwargs and defaults (ctc.py:115-145), same
``forward(xs, ys, x_lens, y_lens, is_eval=False)`` contract (numpy in; a
shape-[1] loss tensor in training, a Python float when ``is_eval``), same
``decode`` / ``posteriors`` return conventions, same state_dict keys.

Differences by design (MI355X-first):
  * the CTC loss is the HIP lattice kernel (native_ops.ctc_loss) on the
    batch-major logits -- no [T,B,V] transpose copy, lengths and labels stay on
    device, no host round trip of costs (ctc.py:319-326 did three);
  * the gradient is produced in backward already scaled by grad_output / B
    (the chain rule; SURVEY §8c decision for the unpinned warp-ctc binding);
  * infeasible alignments give cost 0 / gradient 0 (zero_infinity).
"""
import numpy as np
import torch

from .... import native_ops as ops
from ..base import ModelBase, check_recurrences, eval_retry
from ..linear import LinearND
from ..encoders.load_encoder import load
from ..criterion import cross_entropy_label_smoothing
from .decoders.beam_search_decoder import BeamSearchDecoder
from .decoders.greedy_decoder import GreedyDecoder
from .align import align_logits, check_align_labels


class _Head(object):
    """An output layer not applied yet: its input, the LinearND and the input
    dropout handed over by the encoder (CTC._encode(defer_head=True))."""
    __slots__ = ('x', 'fc', 'drop')

    def __init__(self, x, fc, drop):
        self.x, self.fc, self.drop = x, fc, drop


def _concatenate_labels_np(ys, y_lens):
    """ctc.py:532-549 on the host, vectorised: [B, L] padded -> int32 [sum L]."""
    ys = np.asarray(ys)
    y_lens = np.asarray(y_lens).astype(np.int64)
    mask = np.arange(ys.shape[1])[None, :] < y_lens[:, None]
    return np.ascontiguousarray(ys[mask]).astype(np.int32)


class CTCStream(object):
    """Chunk-by-chunk greedy recognition with a unidirectional CTC model
    (CTC.stream): the encoder state (RNNEncoder.forward_chunk) and the label
    of each row's last frame stay on the device between chunks, so a chunk
    costs O(chunk), and the chunks' labels concatenated are what
    ``decode(beam_width=1)`` returns for the whole utterance.

    ``last_logits``: the device logits [B, Tc', V] of the last chunk and
    ``last_lens_np`` their valid lengths (kept for tests)."""

    def __init__(self, model, batch_size):
        self._model = model
        self._state = model.encoder.init_stream(batch_size)
        self.batch_size = self._state.batch_size
        self._prev = torch.full((self.batch_size,), -1, dtype=torch.int32,
                                device=self._state.device)
        self._emitted = [[] for _ in range(self.batch_size)]
        self.last_logits = None
        self.last_lens_np = None

    def _chunk_logits(self, xs_chunk, chunk_lens, final):
        """The chunk through the encoder and the output layers: (logits [B,
        Tc', V], their valid lengths int32 [B]), both on the device."""
        model = self._model
        if model.training:
            raise RuntimeError('%s.feed runs in eval mode only: the model is in training '
                               'mode (call model.eval(); after an optimizer step open a new '
                               'session, its bf16 weight copies would be stale)'
                               % type(self).__name__)
        xs_d = model.np2var(xs_chunk, dtype='float')
        xs, lens_d = model.encoder.forward_chunk(xs_d, chunk_lens, self._state, final=final)
        for i in range(len(model.fc_list)):
            xs = getattr(model, 'fc_' + str(i))(xs)
        logits = model.fc_out(xs)
        if model.logits_temperature != 1:
            logits = logits * (1.0 / model.logits_temperature)
        return logits, lens_d

    @torch.no_grad()
    def feed(self, xs_chunk, chunk_lens, final=False):
        """xs_chunk [B, Tc, F] (numpy or device tensor), chunk_lens [B]: each
        row's valid frames in this chunk (0: nothing for that row); final (bool
        or one per row): the row's utterance ends with this chunk -- required
        for a chunk length that is no multiple of the encoder's subsampling
        stride (RNNEncoder.forward_chunk raises ValueError otherwise).  Returns
        a list of B int64 arrays, the labels this chunk newly emits, in
        decode()'s index space.  One host read: the labels and their counts.
        The model must be in eval mode (RuntimeError otherwise)."""
        logits, lens_d = self._chunk_logits(xs_chunk, chunk_lens, final)
        hyps, hl = ops.ctc_best_path_stream(logits, lens_d, self._prev, 0)
        packed = torch.cat([hl.view(-1, 1), hyps], dim=1).cpu().numpy()
        self.last_logits = logits
        self.last_lens_np = self._state.last_lens_np.copy()
        new = [packed[b, 1:1 + packed[b, 0]].astype(np.int64) - 1 for b in range(self.batch_size)]
        for b, n in enumerate(new):
            if len(n):
                self._emitted[b].append(n)
        return new

    def hyps(self):
        """The labels emitted so far, per row (since the row's last reset)."""
        return [np.concatenate(e) if e else np.zeros(0, np.int64) for e in self._emitted]

    def reset(self, rows=None):
        """Start a new utterance in `rows` (default: every row): zero encoder
        state, no previous label, empty hypothesis."""
        self._state.reset(rows)
        rows = range(self.batch_size) if rows is None else [int(r) for r in rows]
        if len(rows):
            self._prev.index_fill_(0, torch.as_tensor(rows, dtype=torch.int64,
                                                      device=self._prev.device), -1)
        for b in rows:
            self._emitted[b] = []


class CTCBeamStream(CTCStream):
    """Chunk-by-chunk prefix beam search with a unidirectional CTC model
    (CTC.stream with beam_width > 1, an LM weight or an insertion bonus): the
    encoder state and the search state (the beam in rank order, its node pool,
    with an LM the entries' LM states) stay on the device between chunks.  The
    hypotheses and scores of a row's final chunk are what the whole-utterance
    search (native_ops.ctc_beam_search) gives on the session's concatenated
    logits, bit for bit.

    After a feed: ``stable_lens`` int [B] -- that many first labels of each
    row's hypothesis are final: every beam entry starts with them, and every
    later hypothesis descends from a beam entry -- and ``scores`` float32 [B]:
    the hypothesis' score S_t, which carries the LM's <eos> term only on the
    row's final chunk.  ``max_frames``: the encoder output frames one utterance
    may hold between resets (the search's node pool is sized for them)."""

    def __init__(self, model, batch_size, beam_width, rnnlm, alpha, beta, max_frames):
        self._model = model
        self._state = model.encoder.init_stream(batch_size)
        self.batch_size = B = self._state.batch_size
        if model.training:
            raise RuntimeError('CTC.stream runs in eval mode only: call model.eval() first')
        self.max_frames = int(max_frames)
        if self.max_frames < 1:
            raise ValueError('CTC.stream: max_frames = %r' % (max_frames,))
        # the LM weights are read once per session
        lm = dict(rnnlm.device_weights(), weight=float(alpha)) if alpha > 0 else None
        self._search = ops.ctc_beam_stream_state(B, model.num_classes, beam_width, self.max_frames,
                                                 self._state.device, blank=0, normalize=True,
                                                 lm=lm, beta=beta)
        self._frames = np.zeros(B, np.int64)      # encoder output frames per row so far
        self._hyps = [np.zeros(0, np.int64) for _ in range(B)]
        self.stable_lens = np.zeros(B, np.int64)
        self.scores = np.zeros(B, np.float32)
        self.last_logits = None
        self.last_lens_np = None

    @torch.no_grad()
    def feed(self, xs_chunk, chunk_lens, final=False):
        """xs_chunk, chunk_lens, final as CTCStream.feed.  Returns a list of B
        int64 arrays: each row's current best hypothesis IN FULL, in decode()'s
        index space -- not an increment: the best beam entry can change from
        chunk to chunk (``stable()`` is the part that cannot).  From a row's
        final chunk until its reset the row reports the whole-utterance
        search's result.  A feed that would take a row past max_frames raises ValueError before any launch.
        One host read: lengths, stable lengths, scores and labels together."""
        B = self.batch_size
        lens = np.asarray(chunk_lens).astype(np.int64).reshape(-1)
        if len(lens) == B:
            after = self._frames + lens // self._model.encoder.stream_stride
            bad = np.nonzero(after > self.max_frames)[0]
            if len(bad):
                raise ValueError('CTCBeamStream.feed: rows %s would hold %s encoder frames, '
                                 'max_frames = %d (reset the row, or open the session with a '
                                 'larger max_frames)' % (bad.tolist(), after[bad].tolist(),
                                                         self.max_frames))
        logits, lens_d = self._chunk_logits(xs_chunk, chunk_lens, final)
        self._frames += self._state.last_lens_np
        # a row that has had its final chunk keeps reporting its final result until reset
        fin = self._state.final
        fin_d = ops.h2d(fin.astype(np.int32), logits.device) if fin.any() else None
        hyps, hl, scores, sl = ops.ctc_beam_stream_feed(self._search, logits, lens_d, fin_d)
        longest = max(int(self._frames.max()), 1)
        packed = torch.cat([hl.view(-1, 1), sl.view(-1, 1), scores.view(torch.int32).view(-1, 1),
                            hyps[:, :longest]], dim=1).cpu().numpy()
        self.last_logits = logits
        self.last_lens_np = self._state.last_lens_np.copy()
        self.stable_lens = packed[:, 1].astype(np.int64)
        self.scores = np.ascontiguousarray(packed[:, 2]).view(np.float32).copy()
        self._hyps = [packed[b, 3:3 + packed[b, 0]].astype(np.int64) - 1 for b in range(B)]
        return self.hyps()

    def hyps(self):
        """The last feed's result: each row's current best hypothesis."""
        return [h.copy() for h in self._hyps]

    def stable(self):
        """Per row the labels that can no longer change."""
        return [h[:n].copy() for h, n in zip(self._hyps, self.stable_lens)]

    def nbest(self):
        """Per row the beam's entries, best first: a list of (labels int64 in
        decode()'s index space, score S_t)."""
        hyps, lens, scores, counts = [t.cpu().numpy() for t in
                                      ops.ctc_beam_stream_nbest(self._search)]
        return [[(hyps[b, i, :lens[b, i]].astype(np.int64) - 1, float(scores[b, i]))
                 for i in range(counts[b])] for b in range(self.batch_size)]

    def reset(self, rows=None):
        """Start a new utterance in `rows` (default: every row): zero encoder
        state, the search at the empty prefix.  Other rows go on."""
        self._state.reset(rows)
        rows = list(range(self.batch_size)) if rows is None else [int(r) for r in rows]
        if not rows:
            return
        ops.ctc_beam_stream_reset(self._search, rows)
        for b in rows:
            self._frames[b] = 0
            self._hyps[b] = np.zeros(0, np.int64)
            self.stable_lens[b] = 0
            self.scores[b] = 0.0


class CTC(ModelBase):
    """The Connectionist Temporal Classification model (ctc.py:72-113)."""

    def __init__(self, input_size, encoder_type, encoder_bidirectional, encoder_num_units,
                 encoder_num_proj, encoder_num_layers, fc_list, dropout_input, dropout_encoder,
                 num_classes, parameter_init_distribution='uniform', parameter_init=0.1,
                 recurrent_weight_orthogonal=False, init_forget_gate_bias_with_one=True,
                 subsample_list=[], subsample_type='drop', logits_temperature=1, num_stack=1,
                 splice=1, input_channel=1, conv_channels=[], conv_kernel_sizes=[],
                 conv_strides=[], poolings=[], activation='relu', batch_norm=False,
                 label_smoothing_prob=0, weight_noise_std=0, encoder_residual=False,
                 encoder_dense_residual=False):
        super(ModelBase, self).__init__()
        self.model_type = 'ctc'
        self.input_size = input_size
        self.num_stack = num_stack
        self.encoder_type = encoder_type
        self.encoder_num_units = encoder_num_units * (2 if encoder_bidirectional else 1)
        self.fc_list = fc_list
        self.fc_list_sub = []
        self.subsample_list = subsample_list
        self.num_classes = num_classes + 1
        self.logits_temperature = logits_temperature
        self.weight_noise_injection = False
        self.weight_noise_std = float(weight_noise_std)
        self.ls_prob = label_smoothing_prob

        if encoder_type in ['lstm', 'gru', 'rnn']:
            self.encoder = load(encoder_type=encoder_type)(
                input_size=input_size, rnn_type=encoder_type,
                bidirectional=encoder_bidirectional, num_units=encoder_num_units,
                num_proj=encoder_num_proj, num_layers=encoder_num_layers,
                dropout_input=dropout_input, dropout_hidden=dropout_encoder,
                subsample_list=subsample_list, subsample_type=subsample_type, batch_first=True,
                merge_bidirectional=False, pack_sequence=True, num_stack=num_stack,
                splice=splice, input_channel=input_channel, conv_channels=conv_channels,
                conv_kernel_sizes=conv_kernel_sizes, conv_strides=conv_strides,
                poolings=poolings, activation=activation, batch_norm=batch_norm,
                residual=encoder_residual, dense_residual=encoder_dense_residual, nin=0)
        elif encoder_type == 'cnn':                                  # ctc.py:197-209
            assert num_stack == 1 and splice == 1
            self.encoder = load(encoder_type='cnn')(
                input_size=input_size, input_channel=input_channel, conv_channels=conv_channels,
                conv_kernel_sizes=conv_kernel_sizes, conv_strides=conv_strides,
                poolings=poolings, dropout_input=dropout_input, dropout_hidden=dropout_encoder,
                activation=activation, batch_norm=batch_norm)
            # the CNN encoder drops its own output (per-layer dropout): nothing is
            # handed over to the first layer after it
            self.encoder.pending_output_drop = None
        else:
            raise NotImplementedError('encoder_type=%s' % encoder_type)

        # the first layer after the encoder folds the encoder's output dropout
        # into its product (bf16 mode; rnn.py:392-393 semantics, same mask)
        self.encoder.defer_output_dropout = True
        if len(fc_list) > 0:
            for i in range(len(fc_list)):
                din = self.encoder_num_units if i == 0 else fc_list[i - 1]
                if i == 0 and encoder_type == 'cnn':                 # ctc.py:219-220
                    din = self.encoder.output_size
                setattr(self, 'fc_' + str(i), LinearND(din, fc_list[i], dropout=dropout_encoder))
            self.fc_out = LinearND(fc_list[-1], self.num_classes)
        else:
            self.fc_out = LinearND(self.encoder_num_units, self.num_classes)

        # ctc.py:248-264
        self.init_weights(parameter_init, distribution=parameter_init_distribution,
                          ignore_keys=['bias'])
        self.init_weights(0, distribution='constant', keys=['bias'])
        if recurrent_weight_orthogonal and encoder_type != 'cnn':    # ctc.py:256
            self.init_weights(parameter_init, distribution='orthogonal',
                              keys=[encoder_type, 'weight'], ignore_keys=['bias'])
        if init_forget_gate_bias_with_one:
            self.init_forget_gate_bias_with_one()

        self._decode_greedy_np = GreedyDecoder(blank_index=0)
        self._decode_beam_np = BeamSearchDecoder(blank_index=0)
        self.flatten_parameters_()
        self.encoder.__dict__['_owner'] = self

    # ------------------------------------------------------------------
    @eval_retry
    def forward(self, xs, ys, x_lens, y_lens, is_eval=False):
        """ctc.py:272-342."""
        if is_eval:
            self.eval()
        else:
            self.train()
            if self.weight_noise_injection:
                self.inject_weight_noise(mean=0, std=self.weight_noise_std)
        B = len(xs)
        xs_d = self.np2var(xs, dtype='float')
        logits, out_lens_d, perm_d = self._encode(xs_d, x_lens, defer_head=True)
        if self.logits_temperature != 1:
            logits = logits * (1.0 / self.logits_temperature)

        loss = self._ctc_term(logits, out_lens_d, ys, y_lens, self.encoder.last_perm_np, B)
        if is_eval:
            check_recurrences(self)
            return float(loss.item())
        return loss

    def _head_fusable(self, fc):
        """The output layer and the CTC loss can run as one op (LinearCTCFn):
        nothing but the CTC term reads the logits."""
        return (self.logits_temperature == 1 and self.ls_prob == 0 and
                not (self.training and fc.dropout_p > 0))

    def _encode(self, xs, x_lens, is_multi_task=False, defer_head=False):
        """ctc.py:344-396.  defer_head: the output layer(s) whose only consumer
        is the CTC loss are returned as _Head(x, fc, drop) for _ctc_term's
        fused LinearND + CTC op instead of being applied here."""
        if self.encoder_type == 'cnn':
            xs, x_lens, perm_idx = self._encode_cnn(xs, x_lens)
        elif is_multi_task:
            xs, x_lens, xs_sub, x_lens_sub, perm_idx = self.encoder(
                xs, x_lens, volatile=not self.training)
        else:
            xs, x_lens, perm_idx = self.encoder(xs, x_lens, volatile=not self.training)
        # the encoder's output dropout, when handed over, is folded into the
        # first layer that reads xs (LinearND input_drop: same mask)
        pd = self.encoder.pending_output_drop
        self.encoder.pending_output_drop = None
        for i in range(len(self.fc_list)):
            xs = getattr(self, 'fc_' + str(i))(xs, input_drop=pd)
            pd = None
        if defer_head and self._head_fusable(self.fc_out):
            logits = _Head(xs, self.fc_out, pd)
        else:
            logits = self.fc_out(xs, input_drop=pd)
        if is_multi_task:
            for i in range(len(self.fc_list_sub)):
                xs_sub = getattr(self, 'fc_sub_' + str(i))(xs_sub)
            if defer_head and self._head_fusable(self.fc_out_sub):
                logits_sub = _Head(xs_sub, self.fc_out_sub, None)
            else:
                logits_sub = self.fc_out_sub(xs_sub)
            return logits, x_lens, logits_sub, x_lens_sub, perm_idx
        return logits, x_lens, perm_idx

    def _encode_cnn(self, xs, x_lens):
        """ctc.py:360-363 (encoder_type == 'cnn'): the encoder returns (xs, x_lens),
        nothing is sorted and perm_idx is None; the identity is kept as
        ``last_perm_np`` so the label gather and the decoders read rows in place."""
        enc = self.encoder
        if torch.is_tensor(x_lens):
            x_lens = x_lens.detach().cpu().numpy()
        xs, lens = enc(xs, np.asarray(x_lens).astype(np.int64))
        enc.last_lens_np = np.asarray(lens).astype(np.int32)
        enc.last_perm_np = np.arange(len(enc.last_lens_np), dtype=np.int64)
        enc.pending_output_drop = None
        return xs, ops.h2d(enc.last_lens_np, xs.device), None

    def _ctc_term(self, logits, lens_d, ys, y_lens, perm, B):
        """sum_b cost_b / B on the HIP CTC kernel (+ label smoothing, ctc.py:319-337)."""
        ys_s = (np.asarray(ys) + 1)[perm]                      # blank = 0 (ctc.py:300)
        yl_s = np.asarray(y_lens).astype(np.int32)[perm]
        labels = self.np2var(_concatenate_labels_np(ys_s, yl_s))
        yl_d = self.np2var(yl_s)
        max_l = int(yl_s.max()) if len(yl_s) else 0
        if isinstance(logits, _Head):     # LinearND + CTC as one op (no f32 d logits)
            h = logits
            loss, _ = ops.linear_ctc_loss(h.x, h.fc.fc.weight, h.fc.fc.bias, labels, yl_d, lens_d,
                                          max_l, loss_scale=1.0 / B, drop=h.drop)
            return loss
        loss, _ = ops.ctc_loss(logits, labels, yl_d, lens_d, max_l, loss_scale=1.0 / B)
        if self.ls_prob > 0:
            loss_ls = cross_entropy_label_smoothing(
                logits, y_lens=lens_d, label_smoothing_prob=self.ls_prob,
                distribution='uniform', size_average=False) * (1.0 / B)
            loss = loss * (1 - self.ls_prob) + loss_ls
        return loss

    def inject_weight_noise(self, mean, std):
        """base.py:85-99 (Gaussian weight noise; not on the default hot path)."""
        with torch.no_grad():
            self._flat_param.add_(torch.randn_like(self._flat_param) * std + mean)

    def _task_logits(self, xs_d, x_lens, task):
        """ctc.py:423-433 / :478-488: the logits, device lengths and host
        lengths of the head `task` selects.  A model with a sub head: 0 is the
        main head, 1 the sub head, anything else raises; a single-task model
        ignores `task`."""
        if not hasattr(self, 'main_loss_weight'):
            logits, lens_d, _ = self._encode(xs_d, x_lens)
            return logits, lens_d, self.encoder.last_lens_np
        if task not in (0, 1):
            raise NotImplementedError('task index %r (0: main head, 1: sub head)' % (task,))
        logits, lens_d, logits_sub, lens_sub_d, _ = self._encode(xs_d, x_lens, is_multi_task=True)
        if task == 0:
            return logits, lens_d, self.encoder.last_lens_np
        return logits_sub, lens_sub_d, self.encoder.last_lens_sub_np

    def _check_lm(self, rnnlm, lm_weight, insertion_bonus, task):
        """The LM decode's preconditions, checked before the encoder runs (the
        LM against the width of the head `task` selects).  Returns (alpha,
        beta) in effect: alpha is 0 without an LM term."""
        sub = hasattr(self, 'main_loss_weight') and task == 1
        V = self.num_classes_sub if sub else self.num_classes
        BeamSearchDecoder.check_lm(lm_weight, insertion_bonus, rnnlm, V)
        return float(lm_weight), float(insertion_bonus)

    @eval_retry
    @torch.no_grad()
    def decode(self, xs, x_lens, beam_width, max_decode_len=None, min_decode_len=0,
               length_penalty=0, coverage_penalty=0, task_index=0, rnnlm=None, lm_weight=0,
               insertion_bonus=0):
        """ctc.py:398-452.  beam_width == 1: device best path; beam_width > 1:
        device prefix beam search on the raw logits (log-softmax fused, no
        [B, T, V] log-probability tensor).  lm_weight > 0 (with rnnlm, an RNNLM
        of the head's width: num_classes labels + <eos>) and insertion_bonus
        != 0: the prefix search with shallow fusion (csrc/ctc_beam.hip), at any
        beam_width >= 1; LM class c is the class this method returns.  Returns
        (best_hyps [B] object array of int arrays, None, perm_idx)."""
        alpha, beta = self._check_lm(rnnlm, lm_weight, insertion_bonus, task_index)
        self.eval()
        xs_d = self.np2var(xs, dtype='float')
        logits, out_lens_d, _ = self._task_logits(xs_d, x_lens, task_index)
        check_recurrences(self)
        if alpha != 0 or beta != 0:
            best_hyps = self._decode_beam_np(logits, out_lens_d, beam_width=beam_width,
                                             alpha=alpha, beta=beta, normalize=True, rnnlm=rnnlm)
        elif beam_width == 1:
            best_hyps = self._decode_greedy_np(logits, out_lens_d)
        else:
            best_hyps = self._decode_beam_np(logits, out_lens_d, beam_width=beam_width,
                                             normalize=True)
        best_hyps = np.array([h - 1 for h in best_hyps] + [None], dtype=object)[:-1]
        return best_hyps, None, self.encoder.last_perm_np.copy()

    @eval_retry
    @torch.no_grad()
    def align(self, xs, x_lens, ys, y_lens, task_index=0):
        """CTC forced alignment of known transcripts (csrc/ctc_align.hip): the
        best path of ys through the lattice of the head `task_index` selects
        (as in decode()).  ys [B, L] padded, in the index space decode()
        returns (labels from 0), y_lens [B]; both are reordered by the
        encoder's perm_idx, as in error_rate().  Returns (alignments, spans,
        scores, perm_idx): alignments[b] int32 [output frames of b], the label
        of every encoder OUTPUT frame with blank = -1; spans[b] int32 [L_b, 2]
        the first and last frame of every label; scores float32 [B] the path's
        log-probability.  A row with no alignment (more labels plus repeats
        than frames): an empty alignment, [0, 2] spans, -inf.  ValueError
        before the encoder runs: a label outside [0, num_classes), y_lens[b] >
        ys.shape[1], a negative length.  One host read, after the search."""
        sub = hasattr(self, 'main_loss_weight') and task_index == 1
        ys, y_lens = check_align_labels(
            ys, y_lens, (self.num_classes_sub if sub else self.num_classes) - 1)
        self.eval()
        xs_d = self.np2var(xs, dtype='float')
        logits, out_lens_d, _ = self._task_logits(xs_d, x_lens, task_index)
        check_recurrences(self)
        perm = self.encoder.last_perm_np.copy()
        return align_logits(logits, out_lens_d, ys, y_lens, perm) + (perm,)

    def stream(self, batch_size, beam_width=1, rnnlm=None, lm_weight=0, insertion_bonus=0,
               max_frames=4096):
        """Chunk-by-chunk recognition of `batch_size` utterances side by side.
        beam_width == 1 without an LM term or a bonus: a CTCStream (greedy).
        Otherwise a CTCBeamStream: the prefix beam search of decode() with its
        state kept on the device, rnnlm / lm_weight / insertion_bonus as in
        decode(), max_frames the encoder output frames an utterance may hold
        between resets.  Single-task models with a unidirectional LSTM encoder
        and no conv front-end (RNNEncoder.init_stream names what else is
        refused).  ValueError: decode()'s LM preconditions, beam_width outside
        [1, 64].  NotImplementedError: a GRU LM or one deeper than the kernels'
        limit -- a session has no host search.  The model must be in eval
        mode: RuntimeError otherwise, as forward_chunk."""
        if hasattr(self, 'main_loss_weight'):
            raise NotImplementedError('streaming a hierarchical CTC model (its sub-task output) '
                                      'is not supported')
        if not hasattr(self.encoder, 'init_stream'):
            raise NotImplementedError('streaming needs an LSTM encoder, not encoder_type=%s '
                                      '(a conv front-end\'s context crosses chunk boundaries)'
                                      % self.encoder_type)
        alpha, beta = self._check_lm(rnnlm, lm_weight, insertion_bonus, 0)
        if not 1 <= int(beam_width) <= 64:
            raise ValueError('CTC.stream: beam_width = %r outside [1, 64]' % (beam_width,))
        if int(beam_width) == 1 and alpha == 0 and beta == 0:
            st = CTCStream(self, batch_size)      # (refuses an unsupported encoder first)
            if self.training:
                raise RuntimeError('CTC.stream runs in eval mode only: call model.eval() first')
            return st
        return CTCBeamStream(self, batch_size, int(beam_width), rnnlm, alpha, beta, max_frames)

    @eval_retry
    @torch.no_grad()
    def error_rate(self, xs, x_lens, ys, y_lens, beam_width, max_decode_len=None, meter=None,
                   task_index=0, **decode_kwargs):
        """decode() scored against ys without leaving the device: the same
        best path / prefix beam search, the hypotheses kept as device tensors,
        ys [B, L] (padded, the index space decode() returns) and y_lens
        reordered by the decode's perm_idx, and the batch fed to `meter`
        (utils.evaluation.edit_distance.ErrorRateMeter; a throw-away token
        meter when None).  Returns the batch's int32 [B, 5] device tensor
        (distance, sub, ins, del, reference units), rows in perm_idx order.
        decode_kwargs: decode()'s remaining arguments; rnnlm, lm_weight and
        insertion_bonus select the LM search as in decode(), the others do not
        affect CTC decoding."""
        from ....utils.evaluation.edit_distance import ErrorRateMeter, score_decoded
        alpha, beta = self._check_lm(decode_kwargs.get('rnnlm'), decode_kwargs.get('lm_weight', 0),
                                     decode_kwargs.get('insertion_bonus', 0), task_index)
        self.eval()
        xs_d = self.np2var(xs, dtype='float')
        logits, out_lens_d, _ = self._task_logits(xs_d, x_lens, task_index)
        check_recurrences(self)
        lens = out_lens_d.to(logits.device).int()
        if alpha != 0 or beta != 0:
            hyps, hl, _ = self._decode_beam_np.search(
                logits, lens, beam_width=beam_width, alpha=alpha, beta=beta, normalize=True,
                rnnlm=decode_kwargs.get('rnnlm'))
        elif beam_width == 1:
            hyps, hl = ops.ctc_best_path(logits, lens, 0)
        else:
            hyps, hl, _ = ops.ctc_beam_search(logits, lens, int(beam_width), 0, normalize=True)
        if meter is None:
            meter = ErrorRateMeter('token')
        # blank = 0 on the device, labels from 0 in decode()'s index space
        return score_decoded(meter, logits.device, hyps - 1, hl, None, ys, y_lens,
                             self.encoder.last_perm_np)

    @eval_retry
    @torch.no_grad()
    def posteriors(self, xs, x_lens, temperature=1, blank_scale=None, task_idx=0):
        """ctc.py:455-502."""
        self.eval()
        if blank_scale is not None:
            raise NotImplementedError
        xs_d = self.np2var(xs, dtype='float')
        logits, _, lens_np = self._task_logits(xs_d, x_lens, task_idx)
        check_recurrences(self)
        probs = ops.softmax(logits * (1.0 / temperature))
        return self.var2np(probs), np.asarray(lens_np).astype(np.int32).copy(), \
            self.encoder.last_perm_np.copy()

    def decode_from_probs(self, probs, x_lens, beam_width=1, max_decode_len=None, rnnlm=None,
                          lm_weight=0, insertion_bonus=0):
        """ctc.py:504-529.  beam_width == 1 on the host, as the reference;
        beam_width > 1 on the device, fed log(probs + 1e-10) as it stands.
        rnnlm / lm_weight / insertion_bonus as in decode() (the LM against the
        width of probs)."""
        log_probs = np.log(probs + 1e-10)
        BeamSearchDecoder.check_lm(lm_weight, insertion_bonus, rnnlm, int(log_probs.shape[-1]))
        if lm_weight != 0 or insertion_bonus != 0:
            best = self._decode_beam_np(log_probs, x_lens, beam_width=beam_width,
                                        alpha=float(lm_weight), beta=float(insertion_bonus),
                                        rnnlm=rnnlm)
        elif beam_width == 1:
            best = self._decode_greedy_np(log_probs, x_lens)
        else:
            best = self._decode_beam_np(log_probs, x_lens, beam_width=beam_width)
        return np.array([h - 1 for h in best] + [None], dtype=object)[:-1]
