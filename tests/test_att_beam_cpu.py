"""The attention beam search's workspace query and refusals (no GPU needed):
asr_att_beam_ws_bytes is 0 exactly where asr_att_beam_decode is unsupported,
and the workspace holds what DESIGN.md says it holds."""
import ctypes

import pytest

from pytorch_end2end_speech_recognition_amd import _native as N


def _dims(B=32, T=250, E=640, A=128, C=10, K=201, D=320):
    return N.AttDecDims(B, T, E, A, C, K, D, 1, 1.0, 0)


def _ws(d, W=10, V=29, Y=64, Dz=256, max_len=100):
    return N.query('asr_att_beam_ws_bytes', ctypes.byref(d), W, V, Y, Dz, max_len, None)


def test_workspace_covers_record_and_logits():
    d = _dims()
    nb = _ws(d, W=10, V=10001)
    R = 32 * 10
    need = (100 * R * 250 + R * 10001 + 2 * R * (2 * 320 + 640)) * 4
    assert need <= nb <= need + (1 << 20)


@pytest.mark.parametrize('W', [1, 33, 0, -1])
def test_beam_width_outside_2_32_is_refused(W):
    assert _ws(_dims(), W=W) == 0
    assert b'beam_width' in N.lib().asr_last_error()


@pytest.mark.parametrize('W', [2, 32])
def test_beam_width_limits_are_supported(W):
    assert _ws(_dims(), W=W) > 0


def test_conv_channels_and_lds_limits_are_refused():
    assert _ws(_dims(C=17)) == 0
    assert b'conv channels' in N.lib().asr_last_error()
    assert _ws(_dims(T=8000)) == 0            # attention: 2 T floats alone are 64 KB
    assert b'LDS' in N.lib().asr_last_error()
    assert _ws(_dims(K=200)) == 0             # even conv width
