#!/usr/bin/env python
"""Time attention beam search on the device (native_ops.att_decode_beam) beside
the host path (ASR_ATT_BEAM=host: the per-step ops with the beam bookkeeping in
numpy) on the same model and encoder output, on an MI355X.  Not part of
bench.py.

Shapes: B 32, 250 padded frames (lengths 150 .. 250), max_decode_len 100,
encoder width 640, decoder 320, attention 128, bottleneck 256, embedding 64,
10 x 201 location convolution; (W 4, V 29), (W 10, V 29), (W 10, V 10001).
Random weights with the <eos> logit pushed down, so every search runs its 100
steps on both paths.  --ctc-weight L > 0: the joint CTC/attention search
(decode(..., ctc_weight=L)) on a model with a CTC head; 0 (the default): the
attention-only search on the model without one.  One process; per shape
and path: warm-up calls, then wall time around each call with a device synchronisation on both sides (the
host path synchronises by itself at every step), median (min .. max).

--timit: the TIMIT attention recipe's decoder instead (bgru_att_phone61: GRU
encoder with a bridge layer, so encoder width 256 at the decoder; one-layer GRU
decoder 256, attention 128, bottleneck 256, embedding 32, 10 x 201 location
convolution, init_dec_state zero, 61 phones + <eos>); (W 4, V 62), (W 10, V 62);
B, T and max_decode_len as above.  Without it the shapes, the models and the
output are the ones above.

--lm-weight G > 0: shallow fusion (decode(..., rnnlm=, lm_weight=G)) with a
random LSTM language model over the same V classes: --lm-layers x --lm-units
(2 x 512), --lm-embedding (512).  --host_repeats 0 skips the host path.

Writes profiles/att_beam_bench.txt (or --out).
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _time_ms(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times)), float(np.min(times)), float(np.max(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'att_beam_bench.txt'))
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--host_repeats', type=int, default=3)
    ap.add_argument('--max_decode_len', type=int, default=100)
    ap.add_argument('--ctc-weight', type=float, default=0.0)
    ap.add_argument('--timit', action='store_true')
    ap.add_argument('--lm-weight', type=float, default=0.0)
    ap.add_argument('--lm-layers', type=int, default=2)
    ap.add_argument('--lm-units', type=int, default=512)
    ap.add_argument('--lm-embedding', type=int, default=512)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('att_beam_bench: needs an MI355X; a CPU run gives no time')
    from pytorch_end2end_speech_recognition_amd import native_ops as ops
    from pytorch_end2end_speech_recognition_amd.models.pytorch_v3.attention.attention_seq2seq \
        import AttentionSeq2seq
    ops.set_compute_dtype('fp32')
    B, T, S = 32, 250, args.max_decode_len
    rng = np.random.RandomState(0)
    lens = np.sort(rng.randint(150, T + 1, B))[::-1].copy()
    lens[0] = T
    width = 256 if args.timit else 640
    enc_np = rng.uniform(-1, 1, (B, T, width)).astype(np.float32)
    for b in range(B):
        enc_np[b, lens[b]:] = 0
    enc = torch.from_numpy(enc_np).cuda()
    lines = ['# attention beam search, device path beside host path, MI355X; B %d, T %d (lengths '
             '%d .. %d), max_decode_len %d; wall ms per call, median (min .. max) of %d device / '
             '%d host calls after %d warm-up; ctc_weight %g'
             % (B, T, lens.min(), lens.max(), S, args.repeats, args.host_repeats, args.warmup,
                args.ctc_weight)]
    if args.lm_weight > 0:
        lines[0] += '; lm_weight %g, LSTM LM %d x %d, embedding %d' % (
            args.lm_weight, args.lm_layers, args.lm_units, args.lm_embedding)
    joint = dict(ctc_loss_weight=0.2) if args.ctc_weight > 0 else {}
    sizes = dict(encoder_type='lstm', encoder_num_units=320, decoder_type='lstm',
                 decoder_num_units=320, embedding_dim=64, init_dec_state='first')
    shapes = ((4, 29), (10, 29), (10, 10001))
    if args.timit:
        lines[0] += '; TIMIT recipe decoder: GRU 256, encoder width 256 (bridge), embedding 32'
        sizes = dict(encoder_type='gru', encoder_num_units=256, decoder_type='gru',
                     decoder_num_units=256, embedding_dim=32, init_dec_state='zero',
                     bridge_layer=True)
        shapes = ((4, 62), (10, 62))
    for W, V in shapes:
        torch.manual_seed(V + W)
        model = AttentionSeq2seq(
            input_size=40, encoder_bidirectional=True,
            encoder_num_proj=0, encoder_num_layers=1, attention_type='location',
            attention_dim=128, decoder_num_layers=1,
            dropout_input=0, dropout_encoder=0, dropout_decoder=0,
            dropout_embedding=0, num_classes=V - 1, subsample_list=[False],
            bottleneck_dim=256, **sizes, **joint)
        with torch.no_grad():
            model.fc_0_fwd.fc.bias[V - 1] -= 30.0
        model.set_cuda()
        model.eval()
        lm = {}
        if args.lm_weight > 0:
            from pytorch_end2end_speech_recognition_amd.models.pytorch_v3.lm.rnnlm import RNNLM
            rnnlm = RNNLM(V - 1, args.lm_embedding, 'lstm', False, args.lm_units, args.lm_layers,
                          0, 0, 0)
            rnnlm.set_cuda()
            rnnlm.eval()
            lm = dict(rnnlm=rnnlm, lm_weight=args.lm_weight)

        def run(mode):
            os.environ['ASR_ATT_BEAM'] = mode
            with torch.no_grad():
                out = model._decode_infer_beam(enc, lens, W, S, 0, 0, 0,
                                               ctc_weight=args.ctc_weight, **lm)
            assert ops.last_att_beam_path() == mode
            return out

        dev_t = _time_ms(lambda: run('device'), args.warmup, args.repeats)
        if args.host_repeats <= 0:
            lines.append('W %2d V %5d: device %.1f ms (%.1f .. %.1f)' % ((W, V) + dev_t))
            del model
            continue
        host_t = _time_ms(lambda: run('host'), 0 if args.host_repeats == 1 else args.warmup,
                          args.host_repeats)
        hd, _ = run('device')
        hh, _ = run('host')
        same = sum(int(np.array_equal(a, b)) for a, b in zip(hd, hh))
        lines.append('W %2d V %5d: device %.1f ms (%.1f .. %.1f), host %.1f ms (%.1f .. %.1f), '
                     'host / device %.1fx; %d of %d hypotheses equal, mean length %.1f'
                     % ((W, V) + dev_t + host_t +
                        (host_t[0] / dev_t[0], same, B, float(np.mean([len(h) for h in hd])))))
        del model
    os.environ.pop('ASR_ATT_BEAM', None)
    text = '\n'.join(lines) + '\n'
    sys.stdout.write(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
