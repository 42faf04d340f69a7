"""The input-row loader of the fused forward (lstm_fwd_xgx): buffer -> LDS DMA
of each step's input rows into a three-slot ring, three steps ahead.

The loader can only go wrong at the ring's edges (priming, the last steps
where s + 3 >= T) and at odd row geometry (rows past B, widths without the
swizzle, the smallest width, all sixteen DMAs per step), so these shapes cover
exactly those.  For each: the fused path against the GEMM + recurrence path
(ASR_FUSE_XPROJ=0) within the existing bound of
test_fused_input_projection_matches_gemm_path (the bf16 operands are identical,
only the f32 summation order differs), the fused path twice bitwise, and no
recurrence give-up."""
import ctypes

import numpy as np
import pytest
import torch

SHAPES = [(8, 1, 64, 64), (8, 2, 64, 64), (8, 3, 64, 64), (8, 4, 64, 64), (8, 7, 64, 64),
          (13, 40, 256, 120), (9, 33, 64, 8), (16, 24, 512, 1024)]
NAMES = ['y', 'dx', 'dW_ih', 'dW_hh', 'db_ih', 'db_hh']


def _forward_path():
    from pytorch_end2end_speech_recognition_amd import _native as NL
    out = (ctypes.c_int * 2)()
    NL.call('asr_lstm_last_path', ctypes.cast(out, ctypes.c_void_p))
    return out[0]


@pytest.mark.gpu
@pytest.mark.parametrize('B,T,H,Din', SHAPES)
def test_fused_forward_loader(B, T, H, Din, cuda_dev, monkeypatch):
    from pytorch_end2end_speech_recognition_amd import _native as NL
    from pytorch_end2end_speech_recognition_amd import native_ops as ops
    assert NL.query('asr_lstm_forward_x_ok', B, H, Din), 'shape outside the fused path'
    rng = np.random.RandomState(B + T + H + Din)
    lens = np.sort(rng.randint(T // 2, T + 1, B))[::-1].astype(np.int32)
    lens[0] = T
    dev = cuda_dev
    x = torch.from_numpy(rng.randn(B, T, Din).astype(np.float32) * 0.5).to(dev)
    params = [torch.from_numpy(rng.uniform(-a, a, s).astype(np.float32)).to(dev)
              for a, s in ((0.1, (8 * H, Din)), (0.05, (8 * H, H)), (0.1, (8 * H,)), (0.1, (8 * H,)))]
    lens_d = torch.from_numpy(lens).to(dev)
    dy = torch.from_numpy(rng.randn(B, T, 2 * H).astype(np.float32)).to(dev)

    def run(fuse):
        monkeypatch.setenv('ASR_FUSE_XPROJ', fuse)
        ws = [t.clone().requires_grad_(True) for t in params]
        xx = x.clone().requires_grad_(True)
        ops.recurrence_status(dev)                                  # clear
        y = ops.blstm_layer(xx, lens_d, T, *ws)
        path = _forward_path()
        (y * dy).sum().backward()
        torch.cuda.synchronize()
        assert int(ops.recurrence_status(dev).max().item()) == 0, 'a recurrence gave up'
        assert (path == 3) == (fuse == '1'), path                   # 3: fused projection
        return [y.detach().cpu().numpy(), xx.grad.cpu().numpy()] + [w.grad.cpu().numpy() for w in ws]

    ops.set_compute_dtype('bf16')
    try:
        ref = run('0')
        fused = run('1')
        again = run('1')
    finally:
        ops.set_compute_dtype('fp32')
    for n, a, b in zip(NAMES, ref, fused):
        assert np.isfinite(b).all(), n
        err = np.abs(a - b).max() / (np.abs(a).max() + 1e-12)
        print('%s: max-abs error / max-abs value %.3g' % (n, err))
        assert err < 2e-2, (n, err)
    for n, a, b in zip(NAMES, fused, again):
        assert np.array_equal(a, b), n + ': the fused path is not bitwise repeatable'
