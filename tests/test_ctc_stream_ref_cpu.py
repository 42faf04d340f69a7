"""CPU side of tests/test_ctc_stream_gpu.py: the models of tests/ctc_stream_ref.py
are what that file says they are, and the label comparisons of the GPU tests
are decided by the logit bound, not by luck.

The float64 evaluation's smallest top-two logit gap over ALL valid frames of
each model (no frame excluded; the models' and inputs' seeds chosen so) is at
least 4 x the logit bound of either compute type in absolute terms (bound x
the largest |logit|): two GPU evaluations within the bound of float64 then
have float64's argmax at every frame, with a factor 2 to spare, so the
streamed labels must equal decode(beam_width=1)'s.  In bf16 mode the bound is
0.07 to 0.15 of the largest logit (MARGIN 16 x a bf16 constant of 1.4e-3,
compounded over 3 to 6 layers), so the models have two output classes of
mostly opposite sign: gap / bound is printed per model and precision."""
import numpy as np
import pytest
import torch

import ctc_stream_ref as M
import lstm_stream_ref as S


@pytest.mark.parametrize('name', sorted(M.MODELS))
def test_f64_top_two_gap_is_four_times_the_logit_bound(name):
    logits, lens = M.logits_f64(name)
    gap = M.top_two_gap(logits, lens)
    top = max(float(np.abs(logits[b, :n]).max()) for b, n in enumerate(lens))
    for precision in ('fp32', 'bf16'):
        bound = M.logit_bound(name, precision) * top
        print('%s %s: gap %.3e, logit bound %.3e (x %.3e), gap / bound %.2f'
              % (name, precision, gap, bound, top, gap / bound))
        assert gap >= 4 * bound, (name, precision, gap, bound)
    path = [logits[b, :n].argmax(-1) for b, n in enumerate(lens)]
    assert all(len(p) for p in path)
    # the paths exercise the decoder: a label is emitted and the path changes label
    assert any((p != 0).any() for p in path)
    assert any((np.diff(p) != 0).any() for p in path)


@pytest.mark.parametrize('name', sorted(M.MODELS))
def test_models_and_schedules_are_what_the_gpu_tests_assume(name):
    kw, totals, sizes = M.MODELS[name][:3]
    model = M.build(name)
    enc = model.encoder
    assert enc.num_directions == 1 and enc.conv is None
    assert enc.stream_stride == M.stride(name)
    assert enc.fast_impl == (name == 'fast')
    st = M.stride(name)
    assert all(n % st == 0 for n in sizes[:-1]) and sum(sizes) == max(totals)
    if st > 1:
        assert len(set(totals)) == 1 and sizes[-1] % st != 0
    else:
        assert len(set(totals)) == len(totals) == 3 and 0 in sizes
    logits, lens = M.logits_f64(name, model.state_dict())
    np.testing.assert_array_equal(lens, np.asarray(totals) // st)
    assert logits.shape[2] == kw['num_classes'] + 1
    assert S.layer_constant('fp32') < 1e-5 and S.layer_constant('bf16') < 0.05


def _golden_model(name, cls=None, key='kwargs', **over):
    import json
    from conftest import golden
    from pytorch_end2end_speech_recognition_amd.models.pytorch_v3.ctc.ctc import CTC
    kw = dict(json.loads(str(golden(name)[key])), **over)
    torch.manual_seed(1623)
    return (cls or CTC)(**kw)


def test_unsupported_configurations_are_refused_by_name():
    from pytorch_end2end_speech_recognition_amd.models.pytorch_v3.ctc.hierarchical_ctc import \
        HierarchicalCTC
    with pytest.raises(NotImplementedError, match='bidirectional'):
        _golden_model('model_ctc_fast').stream(2)
    with pytest.raises(NotImplementedError, match='rnn_type=gru'):
        _golden_model('model_ctc_gru_fast').stream(2)
    with pytest.raises(NotImplementedError, match='conv front-end'):
        _golden_model('model_vgg_nobn', encoder_bidirectional=False).stream(2)
    with pytest.raises(NotImplementedError, match='conv front-end'):
        _golden_model('model_cnn_ctc', key='prelu/kwargs').stream(2)
    with pytest.raises(NotImplementedError, match='hierarchical'):
        _golden_model('model_uni_hier', HierarchicalCTC).stream(2)
    enc = _golden_model('model_uni_hier', HierarchicalCTC).encoder
    with pytest.raises(NotImplementedError, match='sub-task'):
        enc.init_stream(2)


def test_bad_chunk_lengths_raise_before_any_launch():
    """On the CPU: a launch would raise NativeError (no CPU path), a refusal
    raises ValueError first."""
    model = M.build('drop_b2')
    with pytest.raises(RuntimeError, match='eval mode'):
        model.stream(2)
    model.eval()
    st = model.stream(2)
    xs = torch.zeros(2, 8, 8)
    with pytest.raises(ValueError, match='multiple of the subsampling stride 4'):
        st.feed(xs, [8, 6])
    with pytest.raises(ValueError, match='outside'):
        st.feed(xs, [9, 8])
    with pytest.raises(ValueError, match='rows'):
        st.feed(xs[:1], [8])
    state = model.encoder.init_stream(2)
    state.final[1] = True
    with pytest.raises(ValueError, match='final chunk'):
        model.encoder.forward_chunk(xs, [8, 4], state)
    state.reset(rows=[1])
    assert not state.final.any()
    model.train()
    with pytest.raises(RuntimeError, match='eval mode'):
        model.encoder.forward_chunk(xs, [8, 8], state)
    with pytest.raises(RuntimeError, match='eval mode'):
        st.feed(xs, [8, 8])
