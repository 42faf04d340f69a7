"""RNNLM (models/pytorch_v3/lm/rnnlm.py): the loss and every parameter gradient
against the reference's own computation restated on CPU torch in float64
(torch.nn.Embedding / LSTM or GRU / Linear / cross_entropy), its state_dict
against a torch.nn.LSTM-based twin, checkpoints, a short Adam run, and the
constructor's refusals.

Bound of the gradient check: 16 x the largest absolute error, over the loss and
every gradient element, of the SAME restatement run in f32 against f64,
recomputed by the test (the rule of the beam-search tests).  One number per
case: the device sums in another order than torch's f32 CPU kernels, so its
error is spread differently over the tensors, and the largest element error is
the scale both share."""
import numpy as np
import pytest
import torch
import torch.nn as nn

V, Y, H = 6, 5, 9                 # classes with <eos> = 5, embedding, units
Y_LENS = np.array([7, 4, 2])      # the length 2 gives a one-step row
# name -> (rnn_type, layers, embedding_dim, tie_weights)
CASES = {'lstm1': ('lstm', 1, Y, False), 'lstm2': ('lstm', 2, Y, False),
         'tied': ('lstm', 1, H, True), 'gru': ('gru', 2, Y, False)}


def _ys():
    rng = np.random.RandomState(2)
    ys = np.full((len(Y_LENS), Y_LENS.max()), -1, np.int64)
    for b, n in enumerate(Y_LENS):
        ys[b, 0] = V - 1                              # <sos>
        ys[b, 1:n - 1] = rng.randint(0, V - 1, n - 2)
        ys[b, n - 1] = V - 1                          # <eos>
    return ys


def _lm(name, seed=1623, **over):
    from pytorch_end2end_speech_recognition_amd.models.pytorch_v3.lm.rnnlm import RNNLM
    rnn_type, layers, emb, tied = CASES[name]
    torch.manual_seed(seed)
    kw = dict(num_classes=V - 1, embedding_dim=emb, rnn_type=rnn_type, bidirectional=False,
              num_units=H, num_layers=layers, dropout_embedding=0, dropout_hidden=0,
              dropout_output=0, parameter_init=0.5, tie_weights=tied)
    kw.update(over)
    return RNNLM(**kw)


class Twin(nn.Module):
    """The reference's module tree on plain torch modules."""

    def __init__(self, rnn_type, layers, emb, tied):
        super(Twin, self).__init__()
        self.embed = nn.Module()
        self.embed.embed = nn.Embedding(V, emb, padding_idx=-1)
        cell = nn.LSTM if rnn_type == 'lstm' else nn.GRU
        setattr(self, rnn_type, cell(emb, hidden_size=H, num_layers=layers, batch_first=True))
        self.output = nn.Module()
        self.output.fc = nn.Linear(H, V)
        if tied:
            self.output.fc.weight = self.embed.embed.weight
        self.rnn_type = rnn_type

    def loss(self, ys, y_lens):
        """rnnlm.py:135-209 row by row (what its packed sequence computes)."""
        total = 0
        for b, n in enumerate(y_lens):
            row = torch.as_tensor(ys[b, :n])
            out, _ = getattr(self, self.rnn_type)(self.embed.embed(row[:-1])[None])
            total = total + nn.functional.cross_entropy(self.output.fc(out[0]), row[1:],
                                                        reduction='sum')
        return total / len(y_lens)


def _restate(name, sd, dtype):
    """(loss, {parameter name: gradient}) of the restatement in dtype."""
    twin = Twin(*CASES[name]).to(dtype)
    twin.load_state_dict({k: v.to(dtype) for k, v in sd.items()})
    loss = twin.loss(_ys(), Y_LENS)
    loss.backward()
    return float(loss), {k: p.grad.double().numpy() for k, p in twin.named_parameters()}


@pytest.mark.parametrize('name', list(CASES))
def test_state_dict_equals_the_torch_twin(name):
    lm = _lm(name)
    twin = Twin(*CASES[name])
    assert ({k: tuple(v.shape) for k, v in lm.state_dict().items()} ==
            {k: tuple(v.shape) for k, v in twin.state_dict().items()})
    assert list(lm.state_dict()) == list(twin.state_dict())
    assert lm.num_classes == V
    # biases 0, forget gate 1 on both bias vectors
    if CASES[name][0] == 'lstm':
        for k in ('bias_ih_l0', 'bias_hh_l0'):
            bias = getattr(lm.lstm, k).detach().numpy()
            np.testing.assert_array_equal(bias[H:2 * H], 1.0)
            np.testing.assert_array_equal(np.delete(bias, np.s_[H:2 * H]), 0.0)
    assert float(lm.embed.embed.weight.detach().abs().max()) <= 0.5


def test_refusals():
    with pytest.raises(NotImplementedError, match='bidirectional'):
        _lm('lstm1', bidirectional=True)
    with pytest.raises(NotImplementedError, match='rnn'):
        _lm('lstm1', rnn_type='rnn')
    with pytest.raises(ValueError, match='tied'):
        _lm('lstm1', tie_weights=True)               # H 9 != Y 5
    with pytest.raises(NotImplementedError):
        _lm('lstm1').decode(None, 2, 10)


@pytest.mark.gpu
@pytest.mark.parametrize('name', list(CASES))
def test_loss_and_gradients_against_f64(name, cuda_dev):
    from pytorch_end2end_speech_recognition_amd import native_ops
    native_ops.set_compute_dtype('fp32')
    lm = _lm(name)
    sd = {k: v.detach().clone() for k, v in lm.state_dict().items()}
    l64, g64 = _restate(name, sd, torch.float64)
    l32, g32 = _restate(name, sd, torch.float32)
    err = max([abs(l32 - l64)] + [float(np.abs(g32[k] - g64[k]).max()) for k in g64])
    bound = 16 * err
    lm.set_cuda()
    lm.zero_grad()
    loss = lm(_ys(), Y_LENS)
    loss.backward()
    torch.cuda.synchronize()
    print('rnnlm %s: restatement f32-vs-f64 error %.3e, bound %.3e; loss device %.9f f64 %.9f'
          % (name, err, bound, loss.item(), l64))
    worst = abs(loss.item() - l64)
    names = dict(lm.named_parameters())
    assert set(names) == set(g64)
    for k, p in names.items():
        d = float(np.abs(p.grad.double().cpu().numpy() - g64[k]).max())
        print('rnnlm %s: %s gradient error %.3e' % (name, k, d))
        worst = max(worst, d)
    assert worst <= bound
    assert lm(_ys(), Y_LENS, is_eval=True) == pytest.approx(l64, abs=bound)


@pytest.mark.gpu
def test_step_follows_forward(cuda_dev):
    """step() from the zero state over a row's tokens gives the logits whose
    cross-entropy forward() sums."""
    from pytorch_end2end_speech_recognition_amd import native_ops
    native_ops.set_compute_dtype('fp32')
    lm = _lm('lstm2')
    lm.set_cuda()
    ys = _ys()
    want = lm(ys, Y_LENS, is_eval=True)
    total = 0.0
    for b, n in enumerate(Y_LENS):
        state = None
        for t in range(n - 1):
            lg, state = lm.step(np.array([ys[b, t]]), state)
            total += float(nn.functional.cross_entropy(lg.float().cpu(),
                                                       torch.as_tensor(ys[b, t + 1:t + 2]),
                                                       reduction='sum'))
    assert total / len(Y_LENS) == pytest.approx(want, rel=1e-5)


@pytest.mark.gpu
def test_checkpoint_round_trip(cuda_dev, tmp_path):
    from pytorch_end2end_speech_recognition_amd import native_ops
    native_ops.set_compute_dtype('fp32')
    lm = _lm('tied')
    lm.set_cuda()
    lm.set_optimizer('adam', 1e-3, lr_schedule=False)
    lm.save_checkpoint(str(tmp_path), epoch=1, step=2, lr=1e-3, metric_dev_best=1.0)
    other = _lm('tied', seed=7)
    other.set_cuda()
    assert other.load_checkpoint(str(tmp_path), epoch=1)[:2] == (2, 3)
    for (k, a), (_, b) in zip(lm.state_dict().items(), other.state_dict().items()):
        assert torch.equal(a, b), k
    assert other.output.fc.weight is other.embed.embed.weight
    ys = _ys()
    assert other(ys, Y_LENS, is_eval=True) == lm(ys, Y_LENS, is_eval=True)
    # the reference's layout loads too: a plain torch twin's state_dict
    twin = Twin(*CASES['tied'])
    other.load_state_dict(twin.state_dict())
    for k, v in twin.state_dict().items():
        assert torch.equal(other.state_dict()[k].cpu(), v), k


@pytest.mark.gpu
@pytest.mark.parametrize('mode', ['fp32', 'bf16'])
def test_adam_lowers_the_loss(mode, cuda_dev):
    from pytorch_end2end_speech_recognition_amd import native_ops
    from pytorch_end2end_speech_recognition_amd.models.pytorch_v3.lm.rnnlm import RNNLM
    native_ops.set_compute_dtype(mode)
    try:
        torch.manual_seed(1623)
        lm = RNNLM(27, embedding_dim=16, rnn_type='lstm', bidirectional=False, num_units=32,
                   num_layers=2, dropout_embedding=0.1, dropout_hidden=0.1, dropout_output=0.1)
        lm.set_cuda()
        lm.set_optimizer('adam', 1e-2, weight_decay=1e-8, lr_schedule=False)
        rng = np.random.RandomState(0)
        y_lens = np.array([12, 9])
        ys = np.full((2, 12), -1, np.int64)
        for b, n in enumerate(y_lens):
            ys[b, :n] = np.concatenate([[27], rng.randint(0, 27, n - 2), [27]])
        first = lm(ys, y_lens, is_eval=True)
        for _ in range(30):
            lm.optimizer.zero_grad()
            loss = lm(ys, y_lens)
            loss.backward()
            lm.optimizer.step()
        last = lm(ys, y_lens, is_eval=True)
    finally:
        native_ops.set_compute_dtype('fp32')
    print('rnnlm adam %s: loss %.4f -> %.4f' % (mode, first, last))
    assert np.isfinite(first) and np.isfinite(last) and last < first
