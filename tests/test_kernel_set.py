"""The set of gfx950 kernels the library is built from, per translation unit (the *.kd descriptors of build/obj/*.o),
is exactly tests/golden/kernel_set.txt.  A change that only moves host code (dispatch, planning, launching) passes with the
fixture untouched; a change that adds or drops a kernel variant on purpose regenerates it:

    python tools/device_code_hash.py --names > tests/golden/kernel_set.txt

hipcc cross-compiles without a GPU, so this runs in the CPU suite."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))


def test_built_objects_hold_exactly_the_recorded_kernels():
    from xinvert_amd import build as xbuild
    xbuild.build()                                       # (no-op when the objects are current)
    import device_code_hash
    with open(os.path.join(ROOT, 'tests', 'golden', 'kernel_set.txt')) as fh:
        want = fh.read().split('\n')
    want = [ln for ln in want if ln]
    have = device_code_hash.kernel_names(os.path.join(ROOT, 'build', 'obj'))
    assert len(have) > 400, 'the listing saw only %d kernels' % len(have)
    missing, extra = sorted(set(want) - set(have)), sorted(set(have) - set(want))
    assert not missing and not extra, 'kernels gone: %r; kernels new: %r' % (missing[:5], extra[:5])
    assert have == want                                  # (no duplicates, same order: sorted per unit)
    units = {ln.split(' ', 1)[0] for ln in have}
    assert units == {u[0] for u in xbuild.UNITS}, 'units without a kernel, or objects that are no unit: %r' % (
        units ^ {u[0] for u in xbuild.UNITS})
