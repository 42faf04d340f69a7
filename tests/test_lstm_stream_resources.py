"""The step kernel of csrc/lstm_stream.hip (lstm_stream_step, its bf16 and its
exact-f32 instantiation) compiles for gfx950 with no scratch (private segment
0) and within the LDS budget DESIGN.md states for it: 8 KB of static LDS per
work-group, the four waves' partial sums.  Read from the gfx950 code object's
AMDGPU metadata in the built object, as tests/test_lstm_uni_resources.py does
(CPU only); registers and LDS are printed for DESIGN.md's table."""
import os
import re
import subprocess

import pytest

from test_kernel_resources import BUILD, LLVM

KERNEL = 'lstm_stream_step'
LDS_BUDGET = 8192
FIELDS = ('private_segment_fixed_size', 'vgpr_count', 'sgpr_count', 'group_segment_fixed_size')


def _metadata(tmp_path):
    """{kernel name: {field: value}} of lstm_stream.o's gfx950 code object."""
    src = os.path.join(BUILD, 'lstm_stream.o')
    if not os.path.exists(src):
        pytest.skip('%s not built (run __graft_entry__.build())' % src)
    fat, co = str(tmp_path / 'lstm_stream.fatbin'), str(tmp_path / 'lstm_stream.co')
    subprocess.check_call([os.path.join(LLVM, 'llvm-objcopy'), '--dump-section=.hip_fatbin=' + fat,
                           src])
    subprocess.check_call([os.path.join(LLVM, 'clang-offload-bundler'), '--type=o', '--unbundle',
                           '--input=' + fat, '--output=' + co,
                           '--targets=hipv4-amdgcn-amd-amdhsa--gfx950'])
    notes = subprocess.check_output([os.path.join(LLVM, 'llvm-readelf'), '--notes', co]).decode()
    out = {}
    for block in re.split(r'\n\s+- \.', notes):      # one list entry per kernel
        name = re.search(r'\.name:\s+(\S+)', block)
        if not name or '.private_segment_fixed_size' not in block:
            continue
        vals = {}
        for f in FIELDS:
            m = re.search(r'\.?%s:\s+(\d+)' % f, block)
            if m:
                vals[f] = int(m.group(1))
        out[name.group(1)] = vals
    return out


@pytest.mark.skipif(not os.path.exists(os.path.join(LLVM, 'clang-offload-bundler')),
                    reason='ROCm LLVM tools absent')
def test_step_kernel_uses_no_scratch_and_stays_in_the_lds_budget(tmp_path):
    ks = _metadata(tmp_path)
    hits = {k: v for k, v in ks.items() if re.search(r'\d+%sI' % KERNEL, k)}
    assert len(hits) == 2, 'instantiations of %s in lstm_stream.o: %s' % (KERNEL, sorted(hits))
    for name, v in sorted(hits.items()):
        print('%s: VGPRs %s, SGPRs %s, static LDS %s B, scratch %s B'
              % (name, v.get('vgpr_count'), v.get('sgpr_count'), v.get('group_segment_fixed_size'),
                 v.get('private_segment_fixed_size')))
        assert v['private_segment_fixed_size'] == 0
        assert 0 < v['group_segment_fixed_size'] <= LDS_BUDGET
