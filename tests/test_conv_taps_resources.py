"""The bf16 kf x kt convolution kernels (csrc/conv_taps.hip) use no scratch: the
weight-gradient kernel keeps 2 x kf x kt accumulator fragments per wave (200
registers at 5x5), the first place a spill would show.  Read from the built
object as tests/test_kernel_resources.py does (CPU only)."""
import os
import re

import pytest

from test_kernel_resources import LLVM, _kernels

HOT = [('conv_taps', r'taps_bf16'), ('conv_taps', r'taps_wgrad_bf16')]


@pytest.mark.skipif(not os.path.exists(os.path.join(LLVM, 'clang-offload-bundler')),
                    reason='ROCm LLVM tools absent')
@pytest.mark.parametrize('obj,pat', HOT)
def test_conv_taps_kernels_spill_free(obj, pat, tmp_path):
    ks = _kernels(obj, tmp_path)
    hits = {k: v for k, v in ks.items() if re.search(pat, k)}
    assert len(hits) >= (4 if 'wgrad' in pat else 2), hits
    spilled = {k: v for k, v in hits.items() if v}
    assert not spilled, 'scratch bytes / lane: %s' % spilled
