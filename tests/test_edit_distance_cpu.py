"""The edit-distance restatement (tests/edit_distance_ref.py) against the
reference's recorded compute_wer results, its clean-up steps against
hand-written cases, and the package's host path against the restatement.
No GPU."""
import numpy as np
import pytest

from conftest import golden
import edit_distance_ref as R


@pytest.fixture(scope='module')
def fx():
    return golden('edit_distance')


def test_fixture_condition(fx):
    """>= 64 kept pairs per vocabulary size in {2, 3, 30}, lengths 1..40, and
    the generator says how many it drew and dropped."""
    assert list(fx['vocabs']) == [2, 3, 30]
    for k, V in enumerate(fx['vocabs']):
        sel = fx['vocab'] == V
        assert sel.sum() >= 64
        assert fx['drawn'][k] - fx['dropped'][k] == sel.sum()
    for key in ('ref_lens', 'hyp_lens'):
        assert fx[key].min() >= 1 and fx[key].max() <= 40


def test_restatement_equals_reference(fx):
    """All four numbers on every kept pair."""
    got = R.score(fx['hyp'], fx['hyp_lens'], fx['ref'], fx['ref_lens'])
    np.testing.assert_array_equal(got[:, :4], fx['result'])
    np.testing.assert_array_equal(got[:, 4], fx['ref_lens'])


def test_host_path_equals_restatement(fx):
    """The package's own host scorer (what a refused shape runs)."""
    import ast
    import os
    # native_ops imports the HIP binding; take the host functions alone
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                        'pytorch_end2end_speech_recognition_amd', 'native_ops.py')
    tree = ast.parse(open(path).read())
    keep = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in (
        'edit_clean_host', 'edit_units_host', 'edit_counts_host', 'edit_distance_host')]
    assert len(keep) == 4
    ns = {'np': np}
    exec(compile(ast.Module(body=keep, type_ignores=[]), path, 'exec'), ns)
    got = ns['edit_distance_host'](fx['hyp'], fx['hyp_lens'], fx['ref'], fx['ref_lens'])
    np.testing.assert_array_equal(got[:, :4], fx['result'])
    hyp = [[4, 9, 9, 1, 2, 9, 3, 7, 5], [9, 9], []]
    ref = [[1, 2, 9, 9, 3], [1], [9, 1, 9]]
    for unit in ('token', 'word'):
        kw = dict(unit=unit, eos=7, space=9, token_map=[0, 1, 2, 3, -1])
        np.testing.assert_array_equal(
            ns['edit_distance_host'](hyp, [9, 2, 0], ref, [5, 1, 3], **kw),
            R.score(hyp, [9, 2, 0], ref, [5, 1, 3], **kw))


def test_clean_eos_cut():
    assert R.clean([3, 4, 7, 5, 7], is_hyp=True, eos=7) == [3, 4]
    assert R.clean([7, 3], is_hyp=True, eos=7) == []
    assert R.clean([3, 4, 7, 5], is_hyp=False, eos=7) == [3, 4, 7, 5]     # hypothesis only
    assert R.clean([3, 4, 5, 7], n=2, is_hyp=True, eos=7) == [3, 4]
    assert R.clean([3, -1, 4, -1], is_hyp=True) == [3, 4]                 # padding


def test_clean_deleting_map():
    m = [0, 5, -1, 3]                      # 1 -> 5, 2 deleted, tokens >= 4 unchanged
    assert R.clean([0, 1, 2, 3, 4, 2, 9], token_map=m) == [0, 5, 3, 4, 9]
    # the cut looks at the token before the map, the separator after it
    assert R.clean([1, 5, 1], is_hyp=True, eos=5, token_map=m) == [5]
    assert R.clean([0, 1, 2, 1, 0], space=5, token_map=m) == [0, 5, 0]


def test_clean_separators():
    assert R.clean([9, 9, 1, 9, 9, 9, 2, 3, 9], space=9) == [1, 9, 2, 3]
    assert R.clean([9, 9, 9], space=9) == []
    assert R.clean([1, 2], space=9) == [1, 2]
    # a deleted token between two separators joins them into one run
    assert R.clean([1, 9, 4, 9, 2], space=9, token_map=[0, 1, 2, 3, -1]) == [1, 9, 2]


def test_units():
    assert R.units([1, 9, 2, 3], 'token', 9) == [1, 9, 2, 3]       # separators stay in
    assert R.units([1, 9, 2, 3], 'word', 9) == [(1,), (2, 3)]
    assert R.units([], 'word', 9) == []                            # not ['']


def test_empty_hypothesis_and_reference():
    """The border rule, where the reference raises."""
    assert R.counts([1, 2, 3], []) == (3, 0, 0, 3)
    assert R.counts([], [1, 2]) == (2, 0, 2, 0)
    assert R.counts([], []) == (0, 0, 0, 0)
    np.testing.assert_array_equal(
        R.score([[7, 1]], [2], [[1, 2, 3]], [3], eos=7), [[3, 0, 0, 3, 3]])


def test_preference_order():
    """Insertion before substitution before deletion on ties."""
    assert R.counts([0], [1, 0]) == (1, 0, 1, 0)
    assert R.counts([0, 1], [1]) == (1, 0, 0, 1)
    # d = 2 by two substitutions or by one insertion and one deletion: at (2, 2)
    # the insertion test (d[2][1] + 1 == d[2][2]) comes first
    assert R.counts([0, 1], [1, 0]) == (2, 0, 1, 1)
