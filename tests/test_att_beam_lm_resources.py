"""The shallow-fusion kernels of csrc/att_beam.hip (beam_lm_cell, beam_lm_score,
beam_select_lm and its joint form beam_select_ctc_lm) compile for gfx950 with no
scratch (private segment 0).  Read from the gfx950 code object's AMDGPU metadata
in the built object, as tests/test_kernel_resources.py does (CPU only); the
registers and static LDS are printed for DESIGN.md's table."""
import os
import re
import subprocess

import pytest

from test_kernel_resources import BUILD, LLVM

KERNELS = ['beam_lm_cell', 'beam_lm_score', 'beam_select_lm', 'beam_select_ctc_lm']
FIELDS = ('private_segment_fixed_size', 'vgpr_count', 'sgpr_count', 'group_segment_fixed_size')


def _metadata(tmp_path):
    """{kernel name: {field: value}} of att_beam.o's gfx950 code object."""
    src = os.path.join(BUILD, 'att_beam.o')
    if not os.path.exists(src):
        pytest.skip('%s not built (run __graft_entry__.build())' % src)
    fat, co = str(tmp_path / 'att_beam.fatbin'), str(tmp_path / 'att_beam.co')
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
@pytest.mark.parametrize('kernel', KERNELS)
def test_lm_kernels_use_no_scratch(kernel, tmp_path):
    ks = _metadata(tmp_path)
    hits = {k: v for k, v in ks.items() if re.search(r'\d+%sE' % kernel, k)}
    assert len(hits) == 1, 'kernel %s in att_beam.o: %s' % (kernel, sorted(hits))
    (name, v), = hits.items()
    print('%s: VGPRs %s, SGPRs %s, static LDS %s B, scratch %s B'
          % (kernel, v.get('vgpr_count'), v.get('sgpr_count'), v.get('group_segment_fixed_size'),
             v.get('private_segment_fixed_size')))
    assert v['private_segment_fixed_size'] == 0
