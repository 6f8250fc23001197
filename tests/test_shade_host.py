"""The shading oracle of an instanced scene (tests/shade_common.py), without a
GPU: the non-vacuity conditions of test_shade_gpu.py's instanced cases, on the
oracle alone with M from rt_affine_inverse. The floors sit 20-40 % under what
the scene gave when it was chosen (97x50: 3248 plane and 708 model pixels, 110 /
142 / 104 / 352 / 0 per instance, 564 pixels changed by the shadow switch and
1646 by the reflection switch); the exact M may move a silhouette pixel or two,
not hundreds.
"""
import functools

import numpy as np
import pytest

import shade_common as SC
import shading_ref as SR


@functools.lru_cache(maxsize=None)
def _frames(rt, frame):
    """{(tree, shadows, reflections): oracle result} of the four Lambert
    switch settings of one frame under light "std", flat and tree."""
    (W, H), pos = SC.FRAMES[frame]
    o, d = SC.eye_rays(W, H, pos)
    flat, tree = SC.host_oracles(rt)
    return {(k, sh, rf): SC.shade(base, SC.PLANE, o, d, 0.01, 100.0, "std", SR.LAMBERT, sh, rf)
            for k, base in enumerate((flat, tree)) for sh, rf in SR.LAMBERT_SWITCHES}


def test_the_frame_is_not_vacuous(rt, ref):
    fr = _frames(rt, 0)
    full = fr[(0, True, True)]
    inst = np.where(full.prim >= 0, full.prim >> 32, -1)
    per = [int((inst == k).sum()) for k in range(5)]
    fig = dict(plane=int((full.prim == -2).sum()), model=int((full.prim >= 0).sum()),
               shadow=int((full.color != fr[(0, False, True)].color).sum()),
               refl=int((full.color != fr[(0, True, False)].color).sum()))
    print(fig, per)
    assert len(full.prim) == 4850 and 4850 % 64 != 0  # the last wave is partial
    assert fig["plane"] >= 2500 and fig["model"] >= 500
    assert all(p >= 60 for p in per[:4]) and per[4] == 0
    assert fig["shadow"] >= 300 and fig["refl"] >= 1000


@pytest.mark.parametrize("frame", [0, 1])
def test_defined_without_ties_and_flat_equals_tree(rt, ref, frame):
    fr = _frames(rt, frame)
    for sh, rf in SR.LAMBERT_SWITCHES:
        a, b = fr[(0, sh, rf)], fr[(1, sh, rf)]
        assert SR.defined(a.rgba) and a.ok.all()
        assert a.ties == 0 and b.ties == 0
        differ = (a.color != b.color) | (a.t.view(np.uint32) != b.t.view(np.uint32)) | (a.prim != b.prim)
        assert int(differ.sum()) == 0, f"{int(differ.sum())} pixels differ between the flat and the tree composition"
