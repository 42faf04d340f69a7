"""Host logic of the bf16 parameter shadow (native_ops.param_shadow): when a
shadow is trusted.  No kernels run; the GPU test is test_param_shadow_gpu.py."""
import pytest
import torch


@pytest.fixture
def ops():
    from pytorch_end2end_speech_recognition_amd import native_ops
    prev = native_ops.compute_dtype()
    native_ops.set_compute_dtype('bf16')
    yield native_ops
    native_ops.set_compute_dtype('bf16' if prev == native_ops.BF16 else 'fp32')


def _model():
    flat = torch.zeros(256)
    params = [torch.nn.Parameter(torch.zeros(8, 4)), torch.nn.Parameter(torch.zeros(8, 4))]
    for p, o in zip(params, (64, 96)):
        p.data = flat[o:o + 32].view(8, 4)
    w = flat[64:128].view(16, 4)          # a layer's combined [fwd; rev] view
    return flat, params, w


def test_shadow_trusted_only_after_the_step_and_until_a_write(ops, monkeypatch):
    monkeypatch.delenv('ASR_PARAM_SHADOW', raising=False)
    flat, params, w = _model()
    sh = ops.param_shadow(flat)
    assert sh is not None and sh.buf.dtype == torch.bfloat16 and sh.buf.numel() == 256
    assert ops._shadow_rows(w, params) is None            # never written
    sh.buf.copy_(torch.arange(256, dtype=torch.bfloat16))
    ops.param_shadow_written(sh, flat, params)
    rows = ops._shadow_rows(w, params)
    assert rows.shape == (16, 4) and rows.data_ptr() == sh.buf[64:].data_ptr()
    assert ops.param_shadow(flat) is sh                   # one shadow per flat buffer
    with torch.no_grad():
        params[1].mul_(2.0)                               # a parameter's own write
    assert ops._shadow_rows(w, params) is None
    ops.param_shadow_written(sh, flat, params)
    assert ops._shadow_rows(w, params) is not None
    flat[0:4].fill_(1.0)                                  # a write through the flat buffer
    assert ops._shadow_rows(w, params) is None


@pytest.mark.parametrize('how', ['fp32', 'env'])
def test_shadow_void_after_a_step_that_did_not_write_it(how, ops, monkeypatch):
    """The fused optimizer step writes the parameters from native code and
    bumps no version.  A step taken while param_shadow() is None (fp32 mode,
    ASR_PARAM_SHADOW=0) reports itself through param_shadow_skipped: the
    shadow an earlier step wrote is void until a later step writes it again."""
    monkeypatch.delenv('ASR_PARAM_SHADOW', raising=False)
    flat, params, w = _model()
    other, oparams, ow = _model()
    for f, ps in ((flat, params), (other, oparams)):
        ops.param_shadow_written(ops.param_shadow(f), f, ps)
    sh = ops.param_shadow(flat)
    assert ops._shadow_rows(w, params) is not None
    # the step without a shadow: what FlatOptimizer.step does with sh None
    if how == 'fp32':
        ops.set_compute_dtype('fp32')
    else:
        monkeypatch.setenv('ASR_PARAM_SHADOW', '0')
    assert ops.param_shadow(flat) is None
    ops.param_shadow_skipped(flat)
    ops.set_compute_dtype('bf16')
    monkeypatch.delenv('ASR_PARAM_SHADOW', raising=False)
    assert ops._shadow_rows(w, params) is None
    assert ops._shadow_rows(ow, oparams) is not None      # another model's shadow stands
    assert ops.param_shadow(flat) is sh                   # the buffer is kept ...
    assert ops._shadow_rows(w, params) is None            # ... but not trusted yet
    ops.param_shadow_written(sh, flat, params)            # a step that wrote it
    assert ops._shadow_rows(w, params) is not None
    ops.param_shadow_skipped(torch.zeros(4))              # a flat buffer without a shadow: no-op
    assert ops._shadow_rows(w, params) is not None


def test_shadow_off_in_fp32_and_by_switch(ops, monkeypatch):
    flat, params, w = _model()
    monkeypatch.setenv('ASR_PARAM_SHADOW', '0')
    assert ops.param_shadow(flat) is None
    monkeypatch.delenv('ASR_PARAM_SHADOW')
    ops.set_compute_dtype('fp32')
    assert ops.param_shadow(flat) is None
    assert ops._shadow_rows(w.clone(), params) is None    # not a view of a flat buffer
