"""The scene dispatch (csrc/rt_dispatch.h): which kernel template arguments
serve a scene, cell by cell, through the host-only rtx_dispatch_probe. No GPU.

The probe runs the same type-level mapping every launcher goes through and
reports the adapter's scene kind, the LDS stack slot count N and the adapter's
variant: GridS's kMode, OctS's PACK, 0 for MeshS.
"""
import numpy as np
import pytest

import rtamd
from rtamd import _lib

RT_E_STATE = -4
SLOTS = (4, 7, 15, 31)
GRID_BUF, GRID_BRICKED = 1, 2  # rt_scenes.h kGridBuf, kGridBricked
GRID_MODES = (GRID_BUF, GRID_BRICKED, GRID_BUF | GRID_BRICKED)


def probe(kind, maxd, gmode=0):
    out = np.full(3, -7, np.int32)
    rc = rtamd.lib().rtx_dispatch_probe(kind, maxd, gmode, out.ctypes.data)
    return rc, tuple(int(v) for v in out)


@pytest.mark.parametrize("maxd", SLOTS)
def test_mesh_takes_its_slot_count(maxd):
    assert probe(_lib.RT_SCENE_MESH, maxd) == (0, (_lib.RT_SCENE_MESH, maxd, 0))


@pytest.mark.parametrize("maxd", SLOTS)
def test_octree_packs_up_to_seven_slots(maxd):
    assert probe(_lib.RT_SCENE_OCTREE, maxd) == (0, (_lib.RT_SCENE_OCTREE, maxd, 1 if maxd <= 7 else 0))


@pytest.mark.parametrize("gmode", GRID_MODES)
@pytest.mark.parametrize("maxd", (1,) + SLOTS)
def test_grid_takes_its_mode_and_one_slot(gmode, maxd):
    """A grid scene's maxd is 1; whatever it holds, the kernels get one slot."""
    assert probe(_lib.RT_SCENE_GRID, maxd, gmode) == (0, (_lib.RT_SCENE_GRID, 1, gmode))


@pytest.mark.parametrize("kind", [0, -1, 5, 99, _lib.RT_SCENE_INSTANCED])
@pytest.mark.parametrize("maxd", (1,) + SLOTS)
@pytest.mark.parametrize("gmode", (0,) + GRID_MODES)
def test_kinds_without_an_adapter_are_refused(kind, maxd, gmode):
    """Unknown kinds, and the instanced kind (its entries branch off ahead of
    the dispatch): RT_E_STATE with a message, out untouched."""
    rc, out = probe(kind, maxd, gmode)
    assert rc == RT_E_STATE and out == (-7, -7, -7)
    assert rtamd.lib().rt_last_error()
