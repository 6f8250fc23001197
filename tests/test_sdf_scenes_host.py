"""The premises of the device octree build's GPU cases
(test_sdf_octree_device_gpu.py), pinned from the oracle without a GPU: the node
counts and level sizes of the trees, which say what each case reaches in the
build -- levels above 1024 cells make the flag scan cross blocks, the far cube
never refines its root, the corner cube keeps 8-cell levels -- and that
rth::flatten_octree accepts every one of them.
"""
import numpy as np
import pytest

import sdf_scenes_common as SC


@pytest.mark.parametrize("key,depth", sorted(SC.CASES))
def test_oracle_tree_sizes(ref, rt, key, depth):
    count, sizes = SC.CASES[(key, depth)]
    nodes = SC.oracle_nodes(key, depth)
    assert nodes.size == 36 * count
    got = SC.level_sizes(nodes)
    assert sum(got) == count and len(got) <= depth + 1
    if sizes is not None:
        assert got == sizes
    if (key, depth) in SC.LAST_LEVEL:
        assert got[-1] == SC.LAST_LEVEL[(key, depth)] and len(got) == depth + 1
    max_depth, maxd, words = SC.flatten(rt, nodes)
    assert max_depth == len(got) - 1 and maxd >= 4
    off = SC.offsets(nodes)
    assert np.array_equal(words[off != 0, 0], off[off != 0])


def test_scan_crosses_blocks_at_cube_depth_5():
    """two levels above the scan's 1024-cell tile, neither a multiple of it"""
    sizes = SC.CASES[("cube", 5)][1]
    big = [n for n in sizes[:-1] if n > 1024]
    assert sizes[:-1].count(512) == 1 and big == [1664] and sizes[-1] > 1024
    assert all(n % 1024 for n in big + [sizes[-1]])


def test_overflow_cases_overflow_where_they_say():
    """capacity 1097 (spot's depth-4 tree) drops the cube at its last level,
    capacity 100 at an inner one; the corner cube fits both"""
    cube = SC.CASES[("cube", 4)][1]
    assert sum(cube[:-1]) <= 1097 < sum(cube)
    assert sum(cube[:3]) <= 100 < sum(cube[:4])
    assert SC.CASES[("corner_cube", 4)][0] <= 100
