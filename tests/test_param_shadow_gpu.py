"""bf16 parameter shadow (round 6, native_ops.param_shadow).

In bf16 mode the fused optimizer step also writes a bf16 copy of every
parameter it updates, and the next forward's BLSTM layers take their staged
W_ih from it instead of converting W_ih again.  Both roundings are the same
f2bf (csrc/common.h), so training with the shadow must be BITWISE the
training without it; a parameter written by anything but the optimizer step
voids the shadow for its layer.
"""
import numpy as np
import pytest
import torch

from test_grad_buckets_gpu import _batch, _kw
from test_model_ctc import _build


def _train(sd, batch, H, L, steps, poke, monkeypatch, shadow, fc=()):
    from pytorch_end2end_speech_recognition_amd import native_ops
    from pytorch_end2end_speech_recognition_amd.utils.training import training_loop as TL
    monkeypatch.setenv('ASR_PARAM_SHADOW', '1' if shadow else '0')
    m = _build(dict(_kw(H, L), fc_list=list(fc)))
    m.load_state_dict(sd)
    m.set_cuda()
    m.set_optimizer('adam', 1e-3, weight_decay=1e-6)
    native_ops.SHADOW_STATS['hits'] = 0
    native_ops.SHADOW_STATS['linear_hits'] = 0
    losses = []
    for i in range(steps):
        m, lv = TL.train_step(m, batch, clip_grad_norm=5.0)
        losses.append(float(lv))
        if poke and i == steps - 2:
            # an in-place write outside the optimizer step (a schedule that
            # rescales weights, a manual re-init): the shadow must not be used
            name, p = next((n, p) for n, p in m.named_parameters() if 'weight_ih' in n)
            with torch.no_grad():
                p.mul_(0.5)
    torch.cuda.synchronize()
    return (losses, m._flat_param.clone(), native_ops.SHADOW_STATS['hits'],
            native_ops.SHADOW_STATS['linear_hits'])


@pytest.mark.gpu
@pytest.mark.parametrize('poke', [False, True])
def test_shadow_training_bitwise_equals_conversion(poke, cuda_dev, monkeypatch):
    """With a dense staged fc layer (512 -> 640: the linear path reads its
    bf16 weight from the shadow too) between the encoder and the CTC head."""
    from pytorch_end2end_speech_recognition_amd import native_ops
    H, L, steps, fc = 256, 3, 3, (640,)
    native_ops.set_compute_dtype('bf16')
    try:
        torch.manual_seed(1623)
        sd = {k: v.clone()
              for k, v in _build(dict(_kw(H, L), fc_list=list(fc))).state_dict().items()}
        batch = _batch(T=160)
        l0, p0, h0, q0 = _train(sd, batch, H, L, steps, poke, monkeypatch, False, fc)
        l1, p1, h1, q1 = _train(sd, batch, H, L, steps, poke, monkeypatch, True, fc)
    finally:
        native_ops.set_compute_dtype('fp32')
    assert h0 == 0 and q0 == 0
    # every layer of every forward after the first step reads the shadow,
    # except the poked layer's forward right after the poke; the fc layer too
    assert h1 == L * (steps - 1) - (1 if poke else 0), h1
    assert q1 == steps - 1, q1
    assert l0 == l1, (l0, l1)
    assert torch.equal(p0, p1), int((p0 != p1).sum())
    assert np.isfinite(l1).all()


def _forward_loss(m, batch):
    """One forward alone: (loss value, BLSTM shadow hits, linear shadow hits);
    no persistent recurrence may have given up."""
    from pytorch_end2end_speech_recognition_amd import native_ops
    native_ops.SHADOW_STATS['hits'] = 0
    native_ops.SHADOW_STATS['linear_hits'] = 0
    native_ops.recurrence_status(m.device)                   # clear
    loss = m(batch['xs'], batch['ys'], batch['x_lens'], batch['y_lens'])
    st = native_ops.recurrence_status(m.device)
    torch.cuda.synchronize()
    assert int(st.max()) == 0, st.tolist()
    return loss.item(), native_ops.SHADOW_STATS['hits'], native_ops.SHADOW_STATS['linear_hits']


def _mode_switch(sd, batch, H, L, fc, how, monkeypatch, shadow):
    """bf16 step (shadow on) -> one step with the shadow unavailable -> bf16
    forward -> bf16 step -> bf16 forward.  shadow False: ASR_PARAM_SHADOW=0
    throughout (the same arithmetic, every weight converted)."""
    from pytorch_end2end_speech_recognition_amd import native_ops
    from pytorch_end2end_speech_recognition_amd.utils.training import training_loop as TL

    def env(on):
        monkeypatch.setenv('ASR_PARAM_SHADOW', '1' if on and shadow else '0')
    TL.reset_step_stats()
    env(True)
    m = _build(dict(_kw(H, L), fc_list=list(fc)))
    m.load_state_dict(sd)
    m.set_cuda()
    m.set_optimizer('adam', 1e-3, weight_decay=1e-6)
    losses = []
    m, lv = TL.train_step(m, batch, clip_grad_norm=5.0)
    losses.append(float(lv))
    if how == 'env':
        env(False)
    else:
        native_ops.set_compute_dtype('fp32')
    try:
        m, lv = TL.train_step(m, batch, clip_grad_norm=5.0)
    finally:
        native_ops.set_compute_dtype('bf16')
    losses.append(float(lv))
    env(True)
    fwd3 = _forward_loss(m, batch)
    m, lv = TL.train_step(m, batch, clip_grad_norm=5.0)
    losses.append(float(lv))
    fwd5 = _forward_loss(m, batch)
    torch.cuda.synchronize()
    assert TL.STEP_STATS['steps'] == 3 and TL.STEP_STATS['skipped'] == 0, TL.STEP_STATS
    return losses, fwd3, fwd5, m._flat_param.clone()


@pytest.mark.gpu
@pytest.mark.parametrize('how', ['env', 'fp32'])
def test_shadow_void_across_a_step_that_did_not_write_it(how, cuda_dev, monkeypatch):
    """An optimizer step taken with ASR_PARAM_SHADOW=0 or in fp32 mode updates
    the weights and leaves the shadow as it was; the fused kernel bumps no
    tensor version.  The next bf16 forward must convert the weights, not read
    that stale shadow: its loss equals the run without any shadow bit for bit
    and counts no hit.  After one more shadow-writing step the forward reads
    the shadow again (every BLSTM layer and the dense fc layer), still
    bitwise."""
    from pytorch_end2end_speech_recognition_amd import native_ops
    H, L, fc = 256, 3, (640,)
    native_ops.set_compute_dtype('bf16')
    try:
        torch.manual_seed(1623)
        sd = {k: v.clone()
              for k, v in _build(dict(_kw(H, L), fc_list=list(fc))).state_dict().items()}
        batch = _batch(T=160)
        l0, a0, b0, p0 = _mode_switch(sd, batch, H, L, fc, how, monkeypatch, False)
        l1, a1, b1, p1 = _mode_switch(sd, batch, H, L, fc, how, monkeypatch, True)
    finally:
        native_ops.set_compute_dtype('fp32')
    print('\n%s: forward after the unshadowed step %r (no shadow %r); after the next step %r '
          '(no shadow %r)' % (how, a1, a0, b1, b0))
    assert a0[1:] == (0, 0) and b0[1:] == (0, 0)
    assert a1[1:] == (0, 0), a1                  # no hit on the stale shadow
    assert a1[0] == a0[0], (a1, a0)
    assert b1[1:] == (L, 1), b1                  # the shadow is current again
    assert b1[0] == b0[0], (b1, b0)
    assert l1 == l0, (l1, l0)
    assert torch.equal(p0, p1), int((p0 != p1).sum())
    assert np.isfinite(l1).all() and np.isfinite([a1[0], b1[0]]).all()


@pytest.mark.gpu
@pytest.mark.parametrize('kind', ['adam', 'sgd', 'momentum', 'nesterov'])
def test_optimizer_step_writes_the_shadow(kind, cuda_dev, monkeypatch):
    """The shadow the fused step writes is the bf16 rounding of the parameters
    it leaves, element for element -- also for a guarded step that skips the
    update (guard word nonzero): parameters and optimizer state stay, and the
    shadow is rewritten from the parameters as they are (here after an
    in-place poke the previous shadow did not see)."""
    from pytorch_end2end_speech_recognition_amd import native_ops
    from pytorch_end2end_speech_recognition_amd.models.pytorch_v3.base import OPTIMIZER_KINDS
    assert sorted(OPTIMIZER_KINDS) == ['adam', 'momentum', 'nesterov', 'sgd']
    monkeypatch.setenv('ASR_PARAM_SHADOW', '1')
    native_ops.set_compute_dtype('bf16')
    try:
        m = _build(_kw(64, 2))
        m.set_cuda()
        m.set_optimizer(kind, 1e-2, weight_decay=1e-6)
        opt, flat = m.optimizer, m._flat_param
        g = torch.Generator(device='cpu').manual_seed(OPTIMIZER_KINDS[kind])

        def bf16_bits(t):
            return t.detach().to(torch.bfloat16).view(torch.int16)
        for step in range(2):
            m.zero_grad()
            m._flat_grad.copy_(torch.randn(flat.numel(), generator=g))
            before = flat.clone()
            opt.step(max_norm=5.0)
            sh = native_ops.param_shadow(flat)
            torch.cuda.synchronize()
            assert not torch.equal(before, flat)
            assert torch.equal(sh.buf.view(torch.int16), bf16_bits(flat)), step
        # a write the shadow did not see, then a guarded (skipped) step
        p = next(p for n, p in m.named_parameters() if 'weight_ih' in n)
        with torch.no_grad():
            p.mul_(0.5)
        assert not torch.equal(sh.buf.view(torch.int16), bf16_bits(flat))
        state = [t.clone() for t in (flat, opt.m) + ((opt.v,) if opt.v is not None else ())]
        m._flat_grad.copy_(torch.randn(flat.numel(), generator=g))
        guard = torch.tensor([1, 0], dtype=torch.int32, device=cuda_dev)
        opt.step(max_norm=5.0, guard=guard)
        opt.undo_step_count()
        torch.cuda.synchronize()
        after = [flat, opt.m] + ([opt.v] if opt.v is not None else [])
        for a, b in zip(state, after):
            assert torch.equal(a, b)
        assert torch.equal(sh.buf.view(torch.int16), bf16_bits(flat))
        assert native_ops._shadow_rows(p, tuple(m.parameters())) is not None
    finally:
        native_ops.set_compute_dtype('fp32')
