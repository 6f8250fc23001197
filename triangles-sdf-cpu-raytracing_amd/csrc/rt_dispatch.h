// rt_dispatch.h -- which kernel instantiation serves a scene. The rules are
// written here once: the LDS stack slot options 4 / 7 / 15 / 31 (pick_maxd,
// rt_scene.hip, chooses among them), the octree's packed coordinates for up to
// 7 slots, a grid's three launch modes, and the three modes of a ray batch. Every launcher (rt_device.hip,
// rt_instances.hip) passes a generic callable and gets the adapter and the
// slot count as types; rtx_dispatch_probe (rt_scene.hip) reports the same
// mapping to the tests.
#pragma once
#include <type_traits>

#include "../../include/rtamd.h"
#include "rt_scene.h"
#include "rt_shade.h"

namespace {

template <int N>
using Slots = std::integral_constant<int, N>;
template <class A>
struct AdapterTag {
  using type = A;
};

// what rtx_dispatch_probe reports of an adapter: its scene kind and its variant
template <class A>
struct AdapterInfo;
template <>
struct AdapterInfo<MeshS> {
  static constexpr int kKind = RT_SCENE_MESH, kVariant = 0;
};
template <int kMode>
struct AdapterInfo<GridS<kMode>> {
  static constexpr int kKind = RT_SCENE_GRID, kVariant = kMode;
};
template <bool PACK>
struct AdapterInfo<OctS<PACK>> {
  static constexpr int kKind = RT_SCENE_OCTREE, kVariant = PACK ? 1 : 0;
};

// f(Slots<N>{}) for the stack slots of a tree scene (rt_scene::maxd)
template <class F>
void with_slots(int maxd, F &&f) {
  switch (maxd) {
    case 4: f(Slots<4>{}); break;
    case 7: f(Slots<7>{}); break;
    case 15: f(Slots<15>{}); break;
    default: f(Slots<31>{}); break;
  }
}

// f(Mode<M>{}) for the mode of a ray batch (kRaysAny / kRaysClosest / kRaysNormal, rt_shade.h)
template <int M>
using Mode = std::integral_constant<int, M>;
template <class F>
void with_mode(int mode, F &&f) {
  switch (mode) {
    case kRaysAny: f(Mode<kRaysAny>{}); break;
    case kRaysClosest: f(Mode<kRaysClosest>{}); break;
    default: f(Mode<kRaysNormal>{}); break;
  }
}

// The mapping on plain values, no device and no live scene needed:
// f(AdapterTag<A>{}, Slots<N>{}) for the adapter A and the slot count N of a
// scene of `kind` with `maxd` slots and, for a grid, launch mode `gmode`
// (rti::grid_mode). False, f not called, for a kind without an adapter.
template <class F>
bool dispatch_types(int kind, int maxd, int gmode, F &&f) {
  switch (kind) {
    case RT_SCENE_MESH:
      with_slots(maxd, [&](auto n) { f(AdapterTag<MeshS>{}, n); });
      return true;
    case RT_SCENE_GRID:  // no traversal stack: one slot
      switch (gmode) {
        case kGridBuf | kGridBricked: f(AdapterTag<GridS<kGridBuf | kGridBricked>>{}, Slots<1>{}); break;
        case kGridBricked: f(AdapterTag<GridS<kGridBricked>>{}, Slots<1>{}); break;
        default: f(AdapterTag<GridS<kGridBuf>>{}, Slots<1>{}); break;
      }
      return true;
    case RT_SCENE_OCTREE:  // OctS<PACK>: packed node coordinates for trees of up to 7 slots
      with_slots(maxd, [&](auto n) { f(AdapterTag<OctS<(decltype(n)::value <= 7)>>{}, n); });
      return true;
    default: return false;
  }
}

inline MeshS make_adapter(AdapterTag<MeshS>, const rt_scene *s, const GridDev &) { return MeshS{rti::mesh_dev(s)}; }
template <int kMode>
GridS<kMode> make_adapter(AdapterTag<GridS<kMode>>, const rt_scene *, const GridDev &gd) {
  return GridS<kMode>{gd};
}
template <bool PACK>
OctS<PACK> make_adapter(AdapterTag<OctS<PACK>>, const rt_scene *s, const GridDev &) {
  return OctS<PACK>{OctDev{s->geo.child.p, s->geo.ovals.p}};
}

// f(adapter value, Slots<N>{}) for scene s; false, f not called, when s has no
// geometry a kernel can take (an instanced scene's entries branch off earlier)
template <class F>
bool dispatch_scene(const rt_scene *s, F &&f) {
  GridDev gd{};
  int gmode = 0;
  if (s->info.kind == RT_SCENE_GRID) {
    gd = rti::grid_dev(s);
    gmode = rti::grid_mode(s, gd);
  }
  return dispatch_types(s->info.kind, s->info.maxd, gmode,
                        [&](auto adapter, auto n) { f(make_adapter(adapter, s, gd), n); });
}

}  // namespace
