"""RNN language model (reference models/pytorch/lm/rnnlm.py) on the HIP ops.

Same constructor, the same state_dict keys and shapes (``embed.embed.weight``,
``lstm.weight_ih_l{l}`` ... / ``gru.*``, ``output.fc.weight`` / ``bias``) and the
same torch RNG consumption at construction, so checkpoints interchange with the
reference.  The ``nn.LSTM`` / ``nn.GRU`` module is a parameter holder only; its
forward never runs.

Labels: ``num_classes + 1`` classes, ``<eos>`` = ``num_classes`` -- the index the
attention models use for both ``sos_0`` and ``eos_0`` -- so LM class c is
attention class c and ``AttentionSeq2seq.decode(..., rnnlm=, lm_weight=)`` fuses
the two without a label map (csrc/att_beam.hip states the search).

``forward`` (rnnlm.py:135-209) steps the layers cell by cell on the autograd
ops (ops.embedding, ops.lstm_cell / ops.gru_cell, ops.dropout, one ops.linear
over all steps, ops.xent): an LM over a transcript's ~100 tokens is not a
training hot path, and no sequence kernel is written for it.

Not supported: ``bidirectional=True`` (a bidirectional LM cannot score a prefix)
and ``rnn_type='rnn'``.
"""
import numpy as np
import torch
import torch.nn as nn

from .... import native_ops as ops
from ..base import ModelBase, check_recurrences
from ..linear import Embedding, LinearND


class RNNLM(ModelBase):
    """rnnlm.py:21-133."""

    def __init__(self, num_classes, embedding_dim, rnn_type, bidirectional, num_units, num_layers,
                 dropout_embedding, dropout_hidden, dropout_output,
                 parameter_init_distribution='uniform', parameter_init=0.1, tie_weights=False,
                 init_forget_gate_bias_with_one=True):
        super(ModelBase, self).__init__()
        if rnn_type not in ('lstm', 'gru', 'rnn'):
            raise ValueError('rnn_type must be "lstm" or "gru" or "rnn".')
        unsupported = []
        if rnn_type == 'rnn':
            unsupported.append('rnn_type=rnn')
        if bidirectional:
            unsupported.append('bidirectional (it cannot score a prefix)')
        if unsupported:
            raise NotImplementedError('MI355X RNNLM: not supported: ' + ', '.join(unsupported))
        self.model_type = 'rnnlm'
        self.embedding_dim = embedding_dim
        self.rnn_type = rnn_type
        self.bidirectional = bidirectional
        self.num_directions = 1
        self.num_units = num_units
        self.num_layers = num_layers
        self.parameter_init = parameter_init
        self.tie_weights = tie_weights
        self.dropout_hidden_p = float(dropout_hidden)

        self.num_classes = num_classes + 1        # <eos>
        self.eos = num_classes
        self.padded_index = -1

        self.embed = Embedding(num_classes=self.num_classes, embedding_dim=embedding_dim,
                               dropout=dropout_embedding, ignore_index=self.padded_index)
        cell = nn.LSTM if rnn_type == 'lstm' else nn.GRU
        setattr(self, rnn_type, cell(embedding_dim, hidden_size=num_units, num_layers=num_layers,
                                     bias=True, batch_first=True, dropout=dropout_hidden,
                                     bidirectional=False))
        self.output = LinearND(num_units, self.num_classes, dropout=dropout_output)
        if tie_weights:                             # rnnlm.py:115-119
            if num_units != embedding_dim:
                raise ValueError(
                    'When using the tied flag, num_units must be equal to embedding_dim')
            self.output.fc.weight = self.embed.embed.weight

        # rnnlm.py:121-133
        self.init_weights(parameter_init, distribution=parameter_init_distribution,
                          ignore_keys=['bias'])
        self.init_weights(0, distribution='constant', keys=['bias'])
        if init_forget_gate_bias_with_one:
            self.init_forget_gate_bias_with_one()
        self.flatten_parameters_()

    def _layer(self, l):
        """(weight_ih, weight_hh, bias_ih, bias_hh) of layer l."""
        rnn = getattr(self, self.rnn_type)
        return tuple(getattr(rnn, '%s_l%d' % (n, l))
                     for n in ('weight_ih', 'weight_hh', 'bias_ih', 'bias_hh'))

    def _cell(self, l, x, h, c):
        if self.rnn_type == 'gru':
            return ops.gru_cell(x, h, *self._layer(l)), c
        return ops.lstm_cell(x, h, c, *self._layer(l))

    def init_state(self, n):
        """The zero state of n rows: (h, c), lists of [n, num_units] per layer."""
        zero = torch.zeros(n, self.num_units, dtype=torch.float32, device=self.device)
        return [zero] * self.num_layers, [zero] * self.num_layers

    def forward(self, ys, y_lens, is_eval=False):
        """rnnlm.py:135-209.  ys [B, T] (padded with -1), y_lens [B].  Inputs
        ys[:, :-1], targets ys[:, 1:] over the first y_lens - 1 steps of each
        row; the summed cross-entropy divided by B (a shape-[1] tensor in
        training, a Python float when is_eval)."""
        if is_eval:
            self.eval()
        else:
            self.train()
        ys = np.asarray(ys).astype(np.int64)
        lens = np.asarray(y_lens).reshape(-1).astype(np.int64) - 1      # without <eos>
        B, S = ys.shape[0], ys.shape[1] - 1
        steps = np.arange(S)[None, :] < lens[:, None]
        # a step past the row's length feeds <eos> (the row no gradient reaches)
        # and has no target: it contributes nothing
        inp = np.where(steps & (ys[:, :-1] >= 0), ys[:, :-1], self.eos)
        tgt = np.where(steps, ys[:, 1:], self.padded_index)
        with torch.set_grad_enabled(not is_eval):
            emb = self.embed(self.np2var(inp, dtype='long'), inp)         # [B, S, Y]
            hs, cs = self.init_state(B)
            hs, cs = list(hs), list(cs)
            p = self.dropout_hidden_p if self.training else 0.0
            outs = []
            for t in range(S):
                x = emb[:, t]
                for l in range(self.num_layers):
                    hs[l], cs[l] = self._cell(l, x, hs[l], cs[l])
                    x = hs[l]
                    if p > 0 and l + 1 < self.num_layers:   # nn.LSTM: between layers only
                        x = ops.dropout(x, p)
                outs.append(x)
            logits = self.output(torch.stack(outs, dim=1))                # [B, S, V]
            loss = ops.xent(logits.view(B * S, -1), self.np2var(tgt.reshape(-1), dtype='long'),
                            ce_scale=1.0 / B)
        if is_eval:
            check_recurrences(self)
            return float(loss.item())
        return loss

    @torch.no_grad()
    def step(self, tokens, state=None):
        """One inference step: tokens int64 [n] (device tensor or array), state
        as init_state (None: the zero state).  Returns (logits [n, V], state)."""
        if not torch.is_tensor(tokens):
            tokens = self.np2var(np.asarray(tokens, np.int64).reshape(-1), dtype='long')
        n = tokens.shape[0]
        hs, cs = self.init_state(n) if state is None else state
        hs, cs = list(hs), list(cs)
        x = ops.embedding(tokens.view(n, 1), self.embed.embed.weight).view(n, -1)
        for l in range(self.num_layers):
            hs[l], cs[l] = self._cell(l, x, hs[l], cs[l])
            x = hs[l]
        logits = ops.linear(x, self.output.fc.weight, self.output.fc.bias)
        return logits, (hs, cs)

    def device_weights(self):
        """The dict native_ops.att_decode_beam(lm=...) takes, without its weight."""
        layers = [self._layer(l) for l in range(self.num_layers)]
        return dict(cell=self.rnn_type, emb=self.embed.embed.weight,
                    w_ih=[w[0] for w in layers], w_hh=[w[1] for w in layers],
                    b_ih=[w[2] for w in layers], b_hh=[w[3] for w in layers],
                    w_out=self.output.fc.weight, b_out=self.output.fc.bias)

    def decode(self, start_token, beam_width, max_decode_len):
        """rnnlm.py:214-225: the reference raises too; the LM decodes inside
        AttentionSeq2seq.decode(..., rnnlm=, lm_weight=)."""
        raise NotImplementedError
