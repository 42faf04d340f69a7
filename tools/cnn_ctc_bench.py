#!/usr/bin/env python
"""Timing record of the pure-CNN CTC recipe (examples/timit/s5/conf/ctc/
cnn_ctc.yml: ten [3, 5] Conv2d layers, 128 -> 256 channels, PReLU, batch norm,
one [3, 1] pool, fc_list [1024] * 3) on the kf x kt convolution kernels.
Nothing is asserted: there is no earlier number for this path.

  1. one training step (forward, CTC loss, backward, clip + Adam) at the
     recipe's own shape -- batch 10, TIMIT-length utterances, input_freq 41 with
     delta and double delta (123 features, from the parent
     blstm_ctc_phone61.yml), 61 phones -- in bf16 mode and in fp32 mode;
  2. the 256 -> 256 [3, 5] layer alone at that step's grid: the new forward,
     input-gradient and weight-gradient kernels against
     torch.nn.functional.conv2d and its autograd (bf16 and f32 tensors, NCHW and
     channels_last) on the same GPU.  The torch figures are the yardstick.

Each figure is the median of REPS timed windows of ITERS calls between device
events, after WARM untimed calls; min and max are printed beside it.  FLOP/s
counts the algorithm's 2 * pixels * Cout * kf * kt * Cin per pass.

Usage (on an MI355X, library built):
    python tools/cnn_ctc_bench.py [--out profiles/cnn_ctc_bench.txt] [--quick]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RECIPE = dict(
    input_freq=41, use_delta=True, use_double_delta=True, input_channel=1, splice=1, num_stack=1,
    encoder_type='cnn', conv_channels=[128] * 4 + [256] * 6, conv_kernel_sizes=[[3, 5]] * 10,
    conv_strides=[[1, 1]] * 10, poolings=[[3, 1]] + [[]] * 9, activation='prelu',
    batch_norm=True, encoder_bidirectional=True, encoder_residual=False,
    encoder_dense_residual=False, encoder_num_units=256, encoder_num_proj=0,
    encoder_num_layers=0, subsample_list=[False], subsample_type='drop',
    fc_list=[1024, 1024, 1024], optimizer='adam', learning_rate=1e-3,
    parameter_init_distribution='uniform', parameter_init=0.1,
    recurrent_weight_orthogonal=True, init_forget_gate_bias_with_one=True, dropout_input=0.2,
    dropout_encoder=0.5, weight_decay=1e-6, logits_temperature=1, label_smoothing_prob=0,
    weight_noise_std=1e-9, num_classes=61)
BATCH = 10
# TIMIT utterances: about 3 s at a 10 ms shift (mean 305 frames); ten fixed lengths
X_LENS = [452, 391, 348, 322, 307, 291, 268, 241, 203, 163]
Y_LENS = [48, 44, 40, 38, 36, 35, 32, 29, 25, 20]


def timed(fn, warm, reps, iters):
    """Median / min / max milliseconds per call over `reps` event-timed windows."""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / iters)
    return float(np.median(ms)), float(min(ms)), float(max(ms))


def step_times(out, quick):
    from pytorch_end2end_speech_recognition_amd import native_ops
    from pytorch_end2end_speech_recognition_amd.models.load_model import load
    from pytorch_end2end_speech_recognition_amd.utils.training.training_loop import train_step
    rng = np.random.RandomState(0)
    T = max(X_LENS)
    xs = rng.randn(BATCH, T, 123).astype(np.float32)
    ys = np.full((BATCH, max(Y_LENS)), -1, np.int32)
    for b in range(BATCH):
        xs[b, X_LENS[b]:] = 0
        ys[b, :Y_LENS[b]] = rng.randint(0, 61, Y_LENS[b])
    batch = dict(xs=xs, ys=ys, x_lens=np.array(X_LENS, np.int32), y_lens=np.array(Y_LENS, np.int32))
    grid = None
    for mode in ('bf16', 'fp32'):
        native_ops.set_compute_dtype(mode)
        torch.manual_seed(1623)
        model = load(model_type='ctc', params=dict(RECIPE), backend='pytorch')
        model.set_cuda()
        model.set_optimizer('adam', 1e-3, weight_decay=1e-6, lr_schedule=False)
        state = {'m': model, 'loss': None}

        def step():
            state['m'], state['loss'] = train_step(state['m'], batch, 5.0)
        warm, reps, iters = (1, 2, 1) if quick or mode == 'fp32' else (3, 5, 3)
        med, lo, hi = timed(step, warm, reps, iters)
        out('train step  %-4s  B=%d T=%d F=123  %9.2f ms  (min %.2f, max %.2f; %d x %d calls, '
            'last loss %.3f)' % (mode, BATCH, T, med, lo, hi, reps, iters, state['loss']))
        grid = (T - 2 * 8, 41)      # the input grid of layer 9 (eight 5-tap layers before it)
        del model, state
        torch.cuda.empty_cache()
    native_ops.set_compute_dtype('fp32')
    return grid


def layer_times(out, grid, quick):
    from pytorch_end2end_speech_recognition_amd import native_ops as ops
    from pytorch_end2end_speech_recognition_amd import _native as N
    dev = torch.device('cuda:0')
    B, (T, F), ci, co, kf, kt = BATCH, grid, 256, 256, 3, 5
    To, Fo = T + 3 - kt, F + 3 - kf
    flops = 2.0 * B * To * Fo * co * kf * kt * ci
    warm, reps, iters = (2, 3, 3) if quick else (5, 7, 10)
    out('layer 256 -> 256, kernel [3, 5] (freq x time), input grid T=%d F=%d, B=%d: '
        '%.2f GFLOP per pass' % (T, F, B, flops / 1e9))
    g = torch.Generator(device='cpu').manual_seed(0)
    x = torch.randn(B, ci, F, T, generator=g)
    w = torch.randn(co, ci, kf, kt, generator=g) * 0.05
    dz = torch.randn(B, co, Fo, To, generator=g)

    def haloed(a):
        Bc, C, f, t = a.shape
        h = torch.zeros(Bc, t + 2, f + 2, C)
        h[:, 1:-1, 1:-1] = a.permute(0, 3, 2, 1)
        return h

    def report(name, fn):
        med, lo, hi = timed(fn, warm, reps, iters)
        out('  %-44s %8.3f ms  (min %.3f, max %.3f)  %7.1f TFLOP/s'
            % (name, med, lo, hi, flops / med / 1e9))

    for mode, cd, dt in (('bf16', ops.BF16, torch.bfloat16), ('fp32', ops.F32, torch.float32)):
        if mode == 'fp32':
            warm, reps, iters = 1, 3, 1
        xh, dzh = haloed(x).to(dev).to(dt), haloed(dz).to(dev).to(dt)
        wd = w.to(dev)
        wg, wt = ops.conv_taps_weight_pack(wd, ci, 0, cd), ops.conv_taps_weight_pack(wd, ci, 1, cd)
        z = torch.zeros(B * (To + 2) * (Fo + 2), co, device=dev)
        dx = torch.zeros(B * (T + 2) * (F + 2), ci, device=dev)
        packed = torch.empty(co, kf * kt * ci, device=dev)
        nb = N.query('asr_conv_taps_wgrad_workspace_bytes', cd, B, T, F, ci, co, kf, kt)
        ws = torch.empty(max(nb, 1), dtype=torch.uint8, device=dev)
        st = N.stream_handle(dev)
        report('asr_conv_taps_forward %s' % mode,
               lambda: ops.conv_taps_forward(xh, B, T, F, ci, wg, co, kf, kt, None, z, cd))
        report('asr_conv_taps_dgrad %s' % mode,
               lambda: ops.conv_taps_dgrad(dzh, B, T, F, ci, wt, co, kf, kt, dx, cd))
        report('asr_conv_taps_wgrad %s' % mode,
               lambda: N.call('asr_conv_taps_wgrad', cd, N.ptr(xh), N.ptr(dzh), B, T, F, ci, co,
                              kf, kt, N.ptr(packed), N.ptr(ws), nb, st))
    warm, reps, iters = (2, 3, 3) if quick else (5, 7, 10)
    Fn = torch.nn.functional
    for dt, name in ((torch.bfloat16, 'bf16'), (torch.float32, 'f32')):
        for fmt, fname in ((torch.contiguous_format, 'NCHW'), (torch.channels_last, 'NHWC')):
            xt = x.to(dev).to(dt).contiguous(memory_format=fmt).requires_grad_(True)
            wt_ = w.to(dev).to(dt).contiguous(memory_format=fmt).requires_grad_(True)
            gz = dz.to(dev).to(dt).contiguous(memory_format=fmt)
            with torch.no_grad():
                report('torch conv2d forward %s %s' % (name, fname),
                       lambda: Fn.conv2d(xt, wt_, padding=1))
            zt = Fn.conv2d(xt, wt_, padding=1)
            report('torch autograd d input %s %s' % (name, fname),
                   lambda: torch.autograd.grad(zt, xt, gz, retain_graph=True))
            report('torch autograd d weight %s %s' % (name, fname),
                   lambda: torch.autograd.grad(zt, wt_, gz, retain_graph=True))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'cnn_ctc_bench.txt'))
    ap.add_argument('--quick', action='store_true', help='fewer repetitions')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('cnn_ctc_bench: no GPU (a timing needs an MI355X)')
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)
    out('# tools/cnn_ctc_bench.py on %s, torch %s' % (torch.cuda.get_device_name(0),
                                                      torch.__version__))
    out('# medians of event-timed windows; measured, nothing asserted')
    grid = step_times(out, args.quick)
    layer_times(out, grid, args.quick)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
