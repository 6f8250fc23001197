// trav_sim.cpp -- where the headline BVH kernel's idle lanes come from, on the CPU.
//
// Rebuilds the bunny's BVH8 through librtamd's host entry points (rt_load_obj,
// rt_bvh_export with the host builder: no GPU), traces the eye rays of one
// orbit frame with the reference traversal (front-to-back, sort8 order,
// per-frame local best, BVHBuilder::traverseNode, triangles_raytracing.cpp:
// 266-335) and records every ray's sequence of loop iterations: I (expand an
// inner node) or L (test a leaf). Each 8x8 wave tile is then replayed in SIMT
// lockstep under issue policies, with a per-iteration cost model in VALU
// instructions (cI inner, cL leaf, cC the shared choose-next part):
//   P0  every iteration runs both branches if any lane needs them (the kernel);
//   P1  one branch per iteration, the one more lanes need (the others wait);
//   P2  leaves wait until no lane needs an inner node (while-while ordering).
// A lane's own visit order never changes under these policies (they only delay
// it), so the results would be the same bits; the question is the cost.
// Output: lane utilisation, wave instructions and iterations per policy.
//
// trav_sim --resume [obj W H]: the loop's second dependent round trip (the
// reload when a frame resumes) under the loop as it was and with the frame
// keeping its second child's entry t; see resume_model below
// (profiles/r07/trav_sim_resume.txt).
//
// trav_sim --share [obj[@N] W H [px py pz]]: per wave-level expansion, the lanes
// that expand and the distinct nodes among them -- what a fetch shared through
// LDS can take off the vector L1; see share_model below
// (profiles/r16/trav_sim_share.txt).
//
// trav_sim --order [obj[@N] W H [px py pz]]: per wave-level expansion, the most
// children any lane enters and whether a lane's entered children tie -- which
// ordering path the expansion takes; see order_model below
// (profiles/r21/trav_sim_order.txt).
//
// build: g++ -O2 -std=c++17 -Iinclude tools/trav_sim.cpp
//          -Ltriangles-sdf-cpu-raytracing_amd/lib -lrtamd -Wl,-rpath,... -o /tmp/trav_sim
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "rtamd.h"

namespace {

struct Node {
  bool leaf;
  uint32_t n;          // children (inner) or index count (leaf)
  uint32_t start;      // leaf: first index position
  float box[48];       // Box8 SoA: mn.x[8] mn.y[8] mn.z[8] mx.x[8] mx.y[8] mx.z[8]
  uint32_t child[8];
};

bool g_split = false;  // leaves of more than 4 triangles as two iterations of one batch each
std::vector<Node> nodes;
std::vector<uint32_t> canon;
std::vector<float> vpos;
std::vector<uint32_t> idx, perm;

uint32_t parse(size_t &at) {
  const uint32_t me = (uint32_t)nodes.size();
  nodes.emplace_back();
  const uint32_t *r = canon.data() + 52 * at;
  ++at;
  Node nd{};
  nd.leaf = r[0] != 0;
  nd.n = r[1];
  nd.start = r[2];
  std::memcpy(nd.box, r + 4, 192);
  if (!nd.leaf)
    for (uint32_t c = 0; c < nd.n; ++c) nd.child[c] = parse(at);
  nodes[me] = nd;
  return me;
}

struct V3 {
  float x, y, z;
};
V3 sub(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
V3 cross(V3 a, V3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
float dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }

float slab(const float *b, int c, V3 o, V3 inv, float tn, float tf) {
  const float t1x = (b[c] - o.x) * inv.x, t2x = (b[24 + c] - o.x) * inv.x;
  const float t1y = (b[8 + c] - o.y) * inv.y, t2y = (b[32 + c] - o.y) * inv.y;
  const float t1z = (b[16 + c] - o.z) * inv.z, t2z = (b[40 + c] - o.z) * inv.z;
  auto mn = [](float a, float b2) { return a < b2 ? a : b2; };
  auto mx = [](float a, float b2) { return a > b2 ? a : b2; };
  float tMin = mx(mn(t1x, t2x), mx(mn(t1y, t2y), mn(t1z, t2z)));
  float tMax = mn(mx(t1x, t2x), mn(mx(t1y, t2y), mx(t1z, t2z)));
  tMin = mx(tMin, tn);
  tMax = mn(tMax, tf);
  return (tMax < 0.0f || tMin > tMax) ? -1.0f : tMin;
}

float tri(uint32_t slot, V3 o, V3 d) {
  const uint32_t *t = idx.data() + 3 * (size_t)perm[slot];
  V3 v[3];
  for (int k = 0; k < 3; ++k) {
    const float *p = vpos.data() + 4 * (size_t)t[k];
    v[k] = {p[0] / p[3], p[1] / p[3], p[2] / p[3]};
  }
  const V3 e1 = sub(v[1], v[0]), e2 = sub(v[2], v[0]);
  const V3 pv = cross(d, e2);
  const float det = dot(e1, pv);
  if (det < 1e-8f && det > -1e-8f) return INFINITY;
  const float inv = 1.0f / det;
  const V3 tv = sub(o, v[0]);
  const float u = dot(tv, pv) * inv;
  const V3 qv = cross(tv, e1);
  const float vv = dot(d, qv) * inv;
  if (u < 0.0f || u > 1.0f || vv < 0.0f || u + vv > 1.0f) return INFINITY;
  return dot(e2, qv) * inv;
}

// traverseNode recursion with the iteration trace: 'I' per inner node, 'L' per leaf
float trace(uint32_t ni, V3 o, V3 d, V3 inv, float tn, float tf, std::string &seq) {
  const Node &nd = nodes[ni];
  float best = INFINITY;
  if (nd.leaf) {
    if (nd.n / 3 > 4) {
      if (g_split) seq += "LL";
      else seq.push_back('M');
    } else {
      seq.push_back('L');
    }
    for (uint32_t k = 0; k < nd.n / 3; ++k) {
      const float t = tri(nd.start / 3 + k, o, d);
      if (t < best) best = t;
    }
    return best;
  }
  seq.push_back('I');
  float t[8];
  int id[8];
  for (int c = 0; c < 8; ++c) {
    t[c] = (uint32_t)c < nd.n ? slab(nd.box, c, o, inv, tn, tf) : -1.0f;
    id[c] = c;
  }
  const int net[19][2] = {{0, 1}, {2, 3}, {4, 5}, {6, 7}, {0, 2}, {1, 3}, {4, 6}, {5, 7}, {1, 2}, {5, 6},
                          {0, 4}, {3, 7}, {1, 5}, {2, 6}, {1, 4}, {3, 6}, {2, 4}, {3, 5}, {3, 4}};
  for (auto &p : net)
    if (t[p[0]] > t[p[1]]) {
      std::swap(t[p[0]], t[p[1]]);
      std::swap(id[p[0]], id[p[1]]);
    }
  for (int i = 0; i < 8; ++i) {
    if (t[i] < 0.0f || (uint32_t)id[i] >= nd.n) continue;
    if (best < t[i]) break;
    const float r = trace(nd.child[id[i]], o, d, inv, tn, tf, seq);
    if (r < best) best = r;
  }
  return best;
}

double g_k = 1.0;  // P1: a side is skipped when the other has more than K times its lanes

struct Cost {
  double lane_instr = 0, wave_instr = 0, iters = 0;
};

// SIMT replay of one tile's sequences under a policy
void replay(const std::vector<std::string> &s, int policy, double cI, double cL, double cC, Cost &out) {
  std::vector<size_t> pos(s.size(), 0);
  for (;;) {
    int nI = 0, nL = 0, live = 0, nM = 0;
    for (size_t k = 0; k < s.size(); ++k) {
      if (pos[k] >= s[k].size()) continue;
      ++live;
      (s[k][pos[k]] == 'I' ? nI : nL)++;
      nM += s[k][pos[k]] == 'M';
    }
    if (!live) break;
    bool runI = nI > 0, runL = nL > 0;
    if (policy == 1 && runI && runL) {  // skip the side with K x fewer lanes
      if (nL * g_k < nI) runL = false;
      else if (nI * g_k < nL) runI = false;
    }
    if (policy == 2 && runI) runL = false;
    double w = cC;
    if (runI) w += cI;
    if (runL) w += nM ? cL : cL / 2;  // a second batch of 4 triangles when any lane's leaf has more
    out.wave_instr += w;
    out.iters += 1;
    // lanes doing useful work: the common part for every lane that advances
    int adv = 0;
    for (size_t k = 0; k < s.size(); ++k) {
      if (pos[k] >= s[k].size()) continue;
      const char c = s[k][pos[k]];
      if ((c == 'I' && runI) || (c != 'I' && runL)) {
        out.lane_instr += (c == 'I' ? cI : c == 'M' ? cL : cL / 2) + cC;
        ++pos[k];
        ++adv;
      }
    }
    (void)adv;
  }
}

// ---- --resume: the kernel's iteration structure, with its second round trip --
// mesh_run (csrc/rt_scenes.h) replayed per ray as a state machine instead of the
// recursion above: one record per loop iteration. An iteration has a top part
// -- expand an inner node (I), test a leaf (L), or nothing (P: the pop-only
// iteration that follows a resume ending in a prune) -- and a "choose the next
// child" tail. The top part's node or triangle fetch is one dependent global
// round trip; a tail that resumes a frame at a child whose entry t is not at
// hand reloads the child's box and word: a second one, exposed after the first.
// Variants (V0 is the loop that ships; V1 to V3 were built, measured slower
// and are no longer in the tree):
//   V0  every resume reloads and recomputes the slab test;
//   V1  the frame keeps its second child's entry t (RT_MESH_T2): a prune there
//       costs no load and the frames below are unwound in the same iteration,
//       a visit loads only the 4-byte child word;
//   V2  V1 + the loads of the frame looked at after a leaf are issued with the
//       leaf's triangle batch (one wait covers both): not exposed.
//   V3  the frame's record in LDS holds its second child's entry t and child
//       word (RT_MESH_T2 = 2): a resume there needs no global load at all; a
//       prune ends the iteration and the next one pops (no unwinding), a
//       visit takes the word from the record
//       (profiles/r10/trav_sim_resume.txt).
// Per ray: round trips by class. Per wave tile (lockstep, the minority side of
// a leaf / inner split waits, as mesh_run does for primary rays): wave iterations, iterations in
// which any advancing lane needs the second round trip, exposed round trips
// (first + second). The cooperative tail is not modelled: its 8-lane groups
// walk the same per-ray sequence.
struct Iter {
  char top;      // 'I', 'L' (leaf, either batch count), 'P'
  bool second;   // the tail needs a global round trip after the top part's
  uint32_t node = 0;  // 'I': the node expanded (--share)
  uint8_t nent = 0;   // 'I': children entered (--order)
  uint8_t tie = 0;    // 'I': bit 0 two entered t equal, bit 1 equal in the top 29 bits (--order)
};
struct RayCounts {
  double inner = 0, leaf = 0, two = 0, pushed = 0, resume_visit = 0, resume_prune = 0, prune_second = 0,
         visit_second = 0, visit_later = 0, pop_only = 0, prune_stored = 0, visit_stored = 0, visit_record = 0, hoisted = 0,
         iters = 0;
};
struct Frame {
  uint32_t node;
  int id[8];
  float t[8];
  int n, next;
  float best;
  uint8_t tie;  // see Iter::tie
};

// the sorted, entered children of an inner node (expand_node)
Frame expand(uint32_t ni, V3 o, V3 inv, float tn, float tf) {
  const Node &nd = nodes[ni];
  float t[8];
  int id[8];
  for (int c = 0; c < 8; ++c) {
    t[c] = (uint32_t)c < nd.n ? slab(nd.box, c, o, inv, tn, tf) : -1.0f;
    id[c] = c;
  }
  const int net[19][2] = {{0, 1}, {2, 3}, {4, 5}, {6, 7}, {0, 2}, {1, 3}, {4, 6}, {5, 7}, {1, 2}, {5, 6},
                          {0, 4}, {3, 7}, {1, 5}, {2, 6}, {1, 4}, {3, 6}, {2, 4}, {3, 5}, {3, 4}};
  for (auto &p : net)
    if (t[p[0]] > t[p[1]]) {
      std::swap(t[p[0]], t[p[1]]);
      std::swap(id[p[0]], id[p[1]]);
    }
  Frame f{};
  f.node = ni;
  f.best = INFINITY;
  for (int i = 0; i < 8; ++i)
    if (!(t[i] < 0.0f) && (uint32_t)id[i] < nd.n) { f.id[f.n] = id[i]; f.t[f.n] = t[i]; ++f.n; }
  for (int i = 1; i < f.n; ++i) {  // sorted: ties are neighbours
    uint32_t a, b;
    std::memcpy(&a, &f.t[i - 1], 4);
    std::memcpy(&b, &f.t[i], 4);
    if (a == b) f.tie |= 1;
    if ((a >> 3) == (b >> 3)) f.tie |= 2;
  }
  return f;
}

// one ray through mesh_run's loop; variant 0 .. 3 as above
void run_ray(V3 o, V3 d, V3 inv, float tn, float tf, int variant, std::vector<Iter> &seq, RayCounts &rc) {
  seq.clear();
  if (nodes[0].leaf) return;
  std::vector<Frame> st;  // st.back() = the top frame (the kernel keeps it in registers)
  Frame root = expand(0, o, inv, tn, tf);  // mesh_root: before the loop, not an iteration
  if (root.n == 0) return;
  rc.two += root.n >= 2;
  st.push_back(root);
  bool have_t = true;
  int64_t word = -1;
  for (;;) {
    Iter it{'P', false, 0};
    if (word >= 0) {
      const Node &nd = nodes[(size_t)word];
      if (nd.leaf) {
        it.top = 'L';
        rc.leaf += 1;
        float lt = INFINITY;
        for (uint32_t k = 0; k < nd.n / 3; ++k) {
          const float t = tri(nd.start / 3 + k, o, d);
          if (lt > t) lt = t;
        }
        if (lt < st.back().best) st.back().best = lt;
      } else {
        it.top = 'I';
        it.node = (uint32_t)word;
        rc.inner += 1;
        Frame f = expand((uint32_t)word, o, inv, tn, tf);
        rc.two += f.n >= 2;
        it.nent = (uint8_t)f.n;
        it.tie = f.tie;
        if (f.n != 0) {
          if (st.back().next == st.back().n) {  // tail call: the top frame is replaced
            if (st.size() >= 2 && st.back().best < st[st.size() - 2].best) st[st.size() - 2].best = st.back().best;
            st.back() = f;
          } else {
            rc.pushed += 1;
            st.push_back(f);
          }
          have_t = true;
        }
      }
      word = -1;
    } else if (!seq.empty() || !have_t) {
      rc.pop_only += 1;
    }
    bool done = false, first = true;
    for (;;) {
      if (st.back().next == st.back().n) {  // frame done: fold into the one below
        const float cb = st.back().best;
        st.pop_back();
        if (st.empty()) { done = true; break; }
        if (cb < st.back().best) st.back().best = cb;
        have_t = false;
      }
      Frame &f = st.back();
      const int k = f.next++;
      const float t = f.t[k];
      const int64_t child = (int64_t)nodes[f.node].child[f.id[k]];
      if (have_t) {  // fresh frame, first child: registers
        have_t = false;
        word = child;
        break;
      }
      const bool covered = variant == 2 && it.top == 'L' && first;  // issued with the leaf's batch
      first = false;
      if (variant >= 1 && k == 1) {  // the stored entry t
        if (f.best < t) {
          rc.prune_stored += 1;
          rc.resume_prune += 1;
          rc.prune_second += 1;
          f.next = f.n;
          if (variant == 3) break;  // the next iteration pops
          continue;  // unwound in this iteration
        }
        rc.visit_stored += 1;
        rc.resume_visit += 1;
        rc.visit_second += 1;
        if (variant == 3) rc.visit_record += 1;  // the word too is in the record: no load
        else if (covered) rc.hoisted += 1;
        else it.second = true;
        word = child;
        break;
      }
      if (covered) rc.hoisted += 1; else it.second = true;
      if (!(f.best < t)) {
        rc.resume_visit += 1;
        (k == 1 ? rc.visit_second : rc.visit_later) += 1;
        word = child;
      } else {
        rc.resume_prune += 1;
        if (k == 1) rc.prune_second += 1;
        f.next = f.n;  // the next iteration pops
      }
      break;
    }
    seq.push_back(it);
    rc.iters += 1;
    if (done) break;
  }
}

struct TileCost {
  double iters = 0, second = 0, exposed = 0, chain = 0;
};

// lockstep replay of one tile under the kernel's majority rule (K = 1)
TileCost replay_resume(const std::vector<std::vector<Iter>> &s) {
  TileCost c;
  std::vector<size_t> pos(s.size(), 0);
  for (auto &q : s) {
    double ch = 0;
    for (auto &i : q) ch += (i.top != 'P') + i.second;
    c.chain = std::max(c.chain, ch);
  }
  for (;;) {
    int nI = 0, nL = 0, live = 0;
    for (size_t k = 0; k < s.size(); ++k) {
      if (pos[k] >= s[k].size()) continue;
      ++live;
      nI += s[k][pos[k]].top == 'I';
      nL += s[k][pos[k]].top == 'L';
    }
    if (!live) break;
    const bool waitL = nL < nI, waitI = !waitL && nI < nL;
    bool top = false, second = false;
    for (size_t k = 0; k < s.size(); ++k) {
      if (pos[k] >= s[k].size()) continue;
      const Iter &i = s[k][pos[k]];
      if ((i.top == 'L' && waitL) || (i.top == 'I' && waitI)) continue;
      top |= i.top != 'P';
      second |= i.second;
      ++pos[k];
    }
    c.iters += 1;
    c.second += second;
    c.exposed += (double)top + (double)second;
  }
  return c;
}

template <class Eye>
int resume_model(Eye eye, V3 org, int W, int H) {
  constexpr int kV = 4;
  const char *vname[kV] = {"V0 every resume reloads", "V1 stored second-child t", "V2 V1 + post-leaf loads hoisted",
                           "V3 second child's t + word in LDS"};
  RayCounts rc[kV];
  std::vector<TileCost> tiles[kV];
  for (int ty = 0; ty < H / 8; ++ty)
    for (int tx = 0; tx < W / 8; ++tx) {
      std::vector<std::vector<Iter>> seqs[kV];
      for (int v = 0; v < kV; ++v) seqs[v].resize(64);
      bool any = false;
      for (int l = 0; l < 64; ++l) {
        const int x = tx * 8 + (l & 7), yo = ty * 8 + (l >> 3), y = H - yo - 1;
        const V3 d = eye(x, y);
        const V3 inv{1.0f / d.x, 1.0f / d.y, 1.0f / d.z};
        for (int v = 0; v < kV; ++v) run_ray(org, d, inv, 0.01f, 100.0f, v, seqs[v][l], rc[v]);
        any |= !seqs[0][l].empty();
      }
      if (!any) continue;
      for (int v = 0; v < kV; ++v) tiles[v].push_back(replay_resume(seqs[v]));
    }
  std::printf("rays %d, wave tiles with a ray past the root %zu\n\n", W * H, tiles[0].size());
  std::printf("per-ray totals (one frame)%34s%14s%14s%14s\n", "V0", "V1", "V2", "V3");
  auto row = [&](const char *n, double RayCounts::*m) {
    std::printf("  %-44s%14.0f%14.0f%14.0f%14.0f\n", n, rc[0].*m, rc[1].*m, rc[2].*m, rc[3].*m);
  };
  row("inner visits below the root (node fetch)", &RayCounts::inner);
  row("leaf visits (triangle batch fetch)", &RayCounts::leaf);
  row("frames with >= 2 entered children", &RayCounts::two);
  row("frames pushed to the LDS stack", &RayCounts::pushed);
  row("resumes that visit the child", &RayCounts::resume_visit);
  row("  at the frame's second child", &RayCounts::visit_second);
  row("  at a third or later child", &RayCounts::visit_later);
  row("resumes that end in a prune", &RayCounts::resume_prune);
  row("  at the frame's second child", &RayCounts::prune_second);
  row("pop-only iterations", &RayCounts::pop_only);
  row("prunes decided from the stored t (no load)", &RayCounts::prune_stored);
  row("visits from the stored t", &RayCounts::visit_stored);
  row("  with the word from the record (no load)", &RayCounts::visit_record);
  row("resume loads issued with a leaf's batch", &RayCounts::hoisted);
  row("lane iterations (with each ray's first)", &RayCounts::iters);
  std::printf("  dependent global round trips per lane chain:\n");
  for (int v = 0; v < kV; ++v) {
    const double resume = rc[v].resume_visit + rc[v].resume_prune - rc[v].prune_stored - rc[v].visit_record;
    const double exposed = resume - rc[v].hoisted;
    const double all = rc[v].inner + rc[v].leaf + exposed;
    std::printf("    %-34s node %.0f + leaf %.0f + resume %.0f (of %.0f loads) = %.0f (resume share %.1f %%)\n", vname[v],
                rc[v].inner, rc[v].leaf, exposed, resume, all, 100.0 * exposed / all);
  }
  // the launch tail: the 1 % of tiles with the most exposed round trips under V0
  std::vector<size_t> order(tiles[0].size());
  for (size_t i = 0; i < order.size(); ++i) order[i] = i;
  std::sort(order.begin(), order.end(), [&](size_t a, size_t b) { return tiles[0][a].exposed > tiles[0][b].exposed; });
  const size_t ntail = std::max<size_t>(1, order.size() / 100);
  std::printf("\nwave tiles in lockstep (minority side waits, K = 1)\n");
  std::printf("  %-34s%12s%16s%16s%16s\n", "", "wave iters", "with 2nd trip", "exposed trips", "longest chain");
  for (int part = 0; part < 2; ++part) {
    std::printf("  %s\n", part == 0 ? "whole frame" : "slowest 1 % of tiles (by V0 exposed trips)");
    double base = 0;
    for (int v = 0; v < kV; ++v) {
      TileCost s;
      const size_t n = part == 0 ? order.size() : ntail;
      for (size_t i = 0; i < n; ++i) {
        const TileCost &t = tiles[v][order[i]];
        s.iters += t.iters; s.second += t.second; s.exposed += t.exposed; s.chain = std::max(s.chain, t.chain);
      }
      if (v == 0) base = s.exposed;
      std::printf("  %-34s%12.0f%16.0f%16.0f%16.0f   (x%.3f exposed vs V0)\n", vname[v], s.iters, s.second, s.exposed,
                  s.chain, s.exposed / base);
    }
  }
  return 0;
}

// ---- --share: how many expansions fetch a node the whole wave shares -------
// The shipped loop (V0, the minority side of a leaf / inner split waits) in
// lockstep per 8x8 wave tile; a frame whose size is no multiple of 8 has
// partial tiles at its right and bottom edges, as the kernels do. For every
// wave-level expansion (an iteration in which at least one lane expands an
// inner node): the lanes that expand and the distinct nodes among them. An
// expansion with one distinct node and at least kShareLanes lanes is what the
// shared fetch (RT_NODE_SHARE, csrc/rt_scenes.h) takes: one 14-lane load and
// 14 LDS broadcasts in place of 14 per-lane vector loads. The cooperative tail
// is not modelled: it starts at 8 rays or fewer, below the threshold.
constexpr int kShareLanes = 14;
struct ShareBin {
  double waves = 0, lanes = 0;
};

template <class Eye>
int share_model(Eye eye, V3 org, int W, int H) {
  // [distinct nodes: 1, 2, 3+][lanes: >= kShareLanes, fewer]
  ShareBin bin[3][2];
  double wave_iters = 0, lane_inner = 0, lane_leaf = 0, busy_tiles = 0, mixed_tiles = 0;
  RayCounts rc;
  for (int ty = 0; ty < (H + 7) / 8; ++ty)
    for (int tx = 0; tx < (W + 7) / 8; ++tx) {
      std::vector<std::vector<Iter>> s(64);
      bool any = false;
      for (int l = 0; l < 64; ++l) {
        const int x = tx * 8 + (l & 7), yo = ty * 8 + (l >> 3), y = H - yo - 1;
        if (x >= W || yo >= H) continue;
        const V3 d = eye(x, y);
        const V3 inv{1.0f / d.x, 1.0f / d.y, 1.0f / d.z};
        run_ray(org, d, inv, 0.01f, 100.0f, 0, s[l], rc);
        any |= !s[l].empty();
      }
      if (!any) continue;
      busy_tiles += 1;
      bool t_shared = false, t_lane = false;
      std::vector<size_t> pos(64, 0);
      for (;;) {
        int nI = 0, nL = 0, live = 0;
        for (int k = 0; k < 64; ++k) {
          if (pos[k] >= s[k].size()) continue;
          ++live;
          nI += s[k][pos[k]].top == 'I';
          nL += s[k][pos[k]].top == 'L';
        }
        if (!live) break;
        const bool waitL = nL < nI, waitI = !waitL && nI < nL;
        std::vector<uint32_t> exp;
        for (int k = 0; k < 64; ++k) {
          if (pos[k] >= s[k].size()) continue;
          const Iter &i = s[k][pos[k]];
          if ((i.top == 'L' && waitL) || (i.top == 'I' && waitI)) continue;
          if (i.top == 'I') exp.push_back(i.node);
          lane_leaf += i.top == 'L';
          ++pos[k];
        }
        wave_iters += 1;
        if (exp.empty()) continue;
        const int n = (int)exp.size();
        std::sort(exp.begin(), exp.end());
        const int dn = (int)(std::unique(exp.begin(), exp.end()) - exp.begin());
        ShareBin &b = bin[std::min(dn, 3) - 1][n >= kShareLanes ? 0 : 1];
        b.waves += 1;
        b.lanes += n;
        lane_inner += n;
        (dn == 1 && n >= kShareLanes ? t_shared : t_lane) = true;
      }
      mixed_tiles += t_shared && t_lane;
    }
  double waves = 0;
  for (auto &r : bin)
    for (auto &b : r) waves += b.waves;
  std::printf("frame %d x %d, rays %d, wave tiles with a ray past the root %.0f, wave iterations %.0f\n", W, H, W * H,
              busy_tiles, wave_iters);
  std::printf("inner visits below the root (lane level) %.0f, leaf visits %.0f\n", lane_inner, lane_leaf);
  std::printf("wave-level expansions %.0f (14 node-vector loads each: %.0f)\n\n", waves, 14 * waves);
  std::printf("%-34s%12s%10s%12s%12s\n", "distinct nodes, expanding lanes", "expansions", "share", "lanes", "lanes/exp");
  const char *dn[3] = {"1 node", "2 nodes", "3+ nodes"};
  for (int d = 0; d < 3; ++d)
    for (int h = 0; h < 2; ++h) {
      const ShareBin &b = bin[d][h];
      char name[64];
      std::snprintf(name, sizeof name, "%s, %s %d lanes", dn[d], h == 0 ? ">=" : "< ", kShareLanes);
      std::printf("%-34s%12.0f%9.1f %%%12.0f%12.1f\n", name, b.waves, waves ? 100.0 * b.waves / waves : 0.0, b.lanes,
                  b.waves ? b.lanes / b.waves : 0.0);
    }
  const double sh = bin[0][0].waves, two = bin[1][0].waves;
  std::printf("\nshared expansions (1 node, >= %d lanes): %.0f of %.0f = %.1f %% of the expansions and of the\n"
              "  frame's node-vector loads; per-lane expansions %.0f; tiles that run both forms %.0f\n",
              kShareLanes, sh, waves, waves ? 100.0 * sh / waves : 0.0, waves - sh, mixed_tiles);
  std::printf("node-vector loads: %.0f -> %.0f (one 14-lane load per shared expansion), LDS reads + %.0f, LDS stores + %.0f\n",
              14 * waves, 14 * (waves - sh) + sh, 14 * sh, sh);
  std::printf("bound for a second round (2 nodes, >= %d lanes): %.0f expansions = %.1f %%\n", kShareLanes, two,
              waves ? 100.0 * two / waves : 0.0);
  return 0;
}

// ---- --order: which ordering path an expansion takes -----------------------
// The same lockstep as --share. Per wave-level expansion: the largest number
// of children any expanding lane enters (the shipped shortcut takes waves with
// at most 2 and no tie), and whether any lane has two entered children with
// equal t, exactly or in the top 29 bits (the keyed order, expand_keyed in
// csrc/rt_scenes.h, sends such a wave to sort8). The same figures over the
// expansions in which a lane of a long ray expands: a ray whose chain is
// kLongChain loop iterations (mesh_run's units of work) or more, the rays a
// launch's tail is made of.
// Then VALU instructions per expansion for the three forms, from the counts
// below (read off `make isa`, render_persist_kernel<MeshS, 4, false>).
constexpr double kLongChain = 64;
struct OrderBin {
  double n = 0, hist[9] = {}, tie_exact = 0, tie29 = 0, le2_notie = 0;
};
// VALU per expansion block. Shipped before round 21: the slab tests and the
// shortcut's test, then the shortcut's tail or the sorted tail. Keyed: 8 slab
// tests of 18 (144), the keys (8), the network (38), the tie check (11), then
// count, list and first t (36); its fallback computes the slab tests again in
// the shipped form (160) and runs the sorted tail. Behind the shortcut (built,
// measured, not kept): the shortcut's test on bit patterns (about 50).
constexpr double kShipCommon = 211, kShipShort = 27, kShipSorted = 137;
constexpr double kKeySlab = 144, kKeyOrder = 93, kKeyShortTest = 50, kKeyShortTail = 24;
constexpr double kKeyFallback = 160 + kShipSorted;

template <class Eye>
int order_model(Eye eye, V3 org, int W, int H) {
  OrderBin all, tail;
  double wave_iters = 0, longest = 0, nlong = 0;
  RayCounts rc;
  for (int ty = 0; ty < (H + 7) / 8; ++ty)
    for (int tx = 0; tx < (W + 7) / 8; ++tx) {
      std::vector<std::vector<Iter>> s(64);
      bool lng[64] = {};
      bool any = false;
      for (int l = 0; l < 64; ++l) {
        const int x = tx * 8 + (l & 7), yo = ty * 8 + (l >> 3), y = H - yo - 1;
        if (x >= W || yo >= H) continue;
        const V3 d = eye(x, y);
        const V3 inv{1.0f / d.x, 1.0f / d.y, 1.0f / d.z};
        run_ray(org, d, inv, 0.01f, 100.0f, 0, s[l], rc);
        any |= !s[l].empty();
        lng[l] = (double)s[l].size() >= kLongChain;
        longest = std::max(longest, (double)s[l].size());
        nlong += lng[l];
      }
      if (!any) continue;
      std::vector<size_t> pos(64, 0);
      for (;;) {
        int nI = 0, nL = 0, live = 0;
        for (int k = 0; k < 64; ++k) {
          if (pos[k] >= s[k].size()) continue;
          ++live;
          nI += s[k][pos[k]].top == 'I';
          nL += s[k][pos[k]].top == 'L';
        }
        if (!live) break;
        const bool waitL = nL < nI, waitI = !waitL && nI < nL;
        int mx = -1, tie = 0;
        bool has_long = false;
        for (int k = 0; k < 64; ++k) {
          if (pos[k] >= s[k].size()) continue;
          const Iter &i = s[k][pos[k]];
          if ((i.top == 'L' && waitL) || (i.top == 'I' && waitI)) continue;
          if (i.top == 'I') {
            mx = std::max(mx, (int)i.nent);
            tie |= i.tie;
            has_long |= lng[k];
          }
          ++pos[k];
        }
        wave_iters += 1;
        if (mx < 0) continue;
        for (OrderBin *b : {&all, has_long ? &tail : (OrderBin *)nullptr}) {
          if (!b) continue;
          b->n += 1;
          b->hist[mx] += 1;
          b->tie_exact += (tie & 1) != 0;
          b->tie29 += (tie & 2) != 0;
          b->le2_notie += mx <= 2 && !(tie & 1);
        }
      }
    }
  std::printf("frame %d x %d, camera (%g, %g, %g), wave iterations %.0f\n", W, H, org.x, org.y, org.z, wave_iters);
  for (int part = 0; part < 2; ++part) {
    const OrderBin &b = part ? tail : all;
    if (part) std::printf("rays of %.0f iterations or more: %.0f (longest ray %.0f); ", kLongChain, nlong, longest);
    std::printf("%s: wave-level expansions %.0f\n", part ? "expansions in which one of them expands" : "whole frame", b.n);
    if (b.n == 0) continue;
    std::printf("  most children any lane enters:");
    for (int i = 0; i <= 8; ++i) std::printf(" %d:%.0f", i, b.hist[i]);
    std::printf("\n  shortcut (<= 2 children, no exact tie) %.0f = %.1f %%, sorted tail %.0f = %.1f %%\n", b.le2_notie,
                100 * b.le2_notie / b.n, b.n - b.le2_notie, 100 * (1 - b.le2_notie / b.n));
    std::printf("  a lane ties exactly %.0f = %.2f %%, in the top 29 bits %.0f = %.2f %% (the keyed order's fallback)\n",
                b.tie_exact, 100 * b.tie_exact / b.n, b.tie29, 100 * b.tie29 / b.n);
    const double ps = b.le2_notie / b.n, pf = b.tie29 / b.n;
    const double ship = kShipCommon + ps * kShipShort + (1 - ps) * kShipSorted;
    const double k1 = kKeySlab + kKeyShortTest + ps * kKeyShortTail + (1 - ps) * kKeyOrder + pf * kKeyFallback;
    const double k2 = kKeySlab + kKeyOrder + pf * kKeyFallback;
    std::printf("  modelled VALU per expansion: shipped %.1f, keys behind the shortcut %.1f, keys only %.1f\n", ship, k1, k2);
    // keys only saves ship - (slab + order) per expansion and pays the fallback
    // on the share pf: level with the shipped form at pf = saving / fallback
    const double S = ship - (kKeySlab + kKeyOrder);
    std::printf("  break-even fallback share, keys only: %.1f / %.0f = %.1f %% of the expansions; here %.2f %%\n", S,
                kKeyFallback, 100 * S / kKeyFallback, 100 * pf);
  }
  return 0;
}

}  // namespace

int main(int argc, char **argv) {
  const bool resume = argc > 1 && std::strcmp(argv[1], "--resume") == 0;
  const bool order = argc > 1 && std::strcmp(argv[1], "--order") == 0;
  const bool share = order || (argc > 1 && std::strcmp(argv[1], "--share") == 0);  // the same arguments
  if (resume || share) { --argc; ++argv; }
  const char *obj = argc > 1 ? argv[1] : "data/_unpacked/stanford-bunny.obj";
  const int W = argc > 2 ? std::atoi(argv[2]) : 1920, H = argc > 3 ? std::atoi(argv[3]) : 1080;
  const double cI = argc > 4 ? std::atof(argv[4]) : 250, cL = argc > 5 ? std::atof(argv[5]) : 360,
               cC = argc > 6 ? std::atof(argv[6]) : 40;
  g_k = argc > 7 ? std::atof(argv[7]) : 1.0;
  g_split = argc > 8 && std::atoi(argv[8]) != 0;
  // "file.obj@N": the mesh subdivided N times (rt_mesh_subdivide; @2 of the
  // bunny is the 1.1 M-triangle stand-in of bench.py's mesh_large)
  std::string path = obj;
  int levels = 0;
  if (const size_t at = path.rfind('@'); at != std::string::npos) {
    levels = std::atoi(path.c_str() + at + 1);
    path.resize(at);
  }
  int64_t nv = 0, ni = 0;
  if (rt_load_obj(path.c_str(), 1, nullptr, &nv, nullptr, &ni)) return std::printf("load: %s\n", rt_last_error()), 1;
  vpos.resize(4 * nv);
  idx.resize(ni);
  rt_load_obj(path.c_str(), 1, vpos.data(), &nv, idx.data(), &ni);
  if (levels > 0) {
    int64_t sv = 0, si = 0;
    if (rt_mesh_subdivide(vpos.data(), nv, idx.data(), ni, levels, nullptr, &sv, nullptr, &si))
      return std::printf("subdivide: %s\n", rt_last_error()), 1;
    std::vector<float> v2(4 * sv);
    std::vector<uint32_t> i2(si);
    rt_mesh_subdivide(vpos.data(), nv, idx.data(), ni, levels, v2.data(), &sv, i2.data(), &si);
    vpos.swap(v2);
    idx.swap(i2);
    nv = sv;
    ni = si;
  }
  rt_set_bvh_builder(RT_BVH_HOST);
  int64_t nn = 0;
  int32_t depth = 0;
  perm.resize(ni / 3);
  rt_bvh_export(vpos.data(), nv, idx.data(), ni, nullptr, &nn, nullptr, &depth);
  canon.resize(52 * nn);
  if (rt_bvh_export(vpos.data(), nv, idx.data(), ni, canon.data(), &nn, perm.data(), &depth))
    return std::printf("export: %s\n", rt_last_error()), 1;
  size_t at = 0;
  parse(at);
  std::printf("%zu nodes, depth %d, %lld tris\n", nodes.size(), depth, (long long)ni / 3);
  // orbit frame 0 of bench.py (pos = (0, 0.5, 2.5)), the kernel's eye rays;
  // --share takes another camera position as its arguments 4 to 6
  float pos[3] = {0.0f, 0.5f, 2.5f};
  const float tgt[3] = {0, 0, 0}, up[3] = {0, 1, 0};
  if (share && argc > 6)
    for (int k = 0; k < 3; ++k) pos[k] = (float)std::atof(argv[4 + k]);
  float vi[16], pi[16];
  rt_camera(pos, tgt, up, 45.0f, (float)W / (float)H, 0.01f, 100.0f, vi, pi);
  auto eye = [&](int x, int y) {
    const float fx = (float)x + 0.5f, fy = (float)y + 0.5f;
    float p[4] = {2.0f * fx / (float)W - 1.0f, 2.0f * fy / (float)H - 1.0f, 0.0f, 1.0f}, q[4];
    for (int r = 0; r < 4; ++r) q[r] = pi[r] * p[0] + pi[4 + r] * p[1] + pi[8 + r] * p[2] + pi[12 + r] * p[3];
    const float w = q[3];
    V3 dd{q[0] / w, q[1] / w, q[2] / w};
    const float l = std::sqrt(dot(dd, dd));
    dd = {dd.x / l, dd.y / l, dd.z / l};
    return V3{vi[0] * dd.x + vi[4] * dd.y + vi[8] * dd.z, vi[1] * dd.x + vi[5] * dd.y + vi[9] * dd.z,
              vi[2] * dd.x + vi[6] * dd.y + vi[10] * dd.z};
  };
  if (resume) return resume_model(eye, V3{pos[0], pos[1], pos[2]}, W, H);
  if (order) return order_model(eye, V3{pos[0], pos[1], pos[2]}, W, H);
  if (share) return share_model(eye, V3{pos[0], pos[1], pos[2]}, W, H);
  Cost c[3];
  double both = 0, iters0 = 0, steps = 0;
  long tiles = 0, busy_tiles = 0, root_only = 0;
  for (int ty = 0; ty < H / 8; ++ty)
    for (int tx = 0; tx < W / 8; ++tx) {
      std::vector<std::string> seqs(64);
      bool any = false;
      for (int l = 0; l < 64; ++l) {
        const int x = tx * 8 + (l & 7), yo = ty * 8 + (l >> 3), y = H - yo - 1;
        const V3 d = eye(x, y);
        const V3 inv{1.0f / d.x, 1.0f / d.y, 1.0f / d.z};
        trace(0, V3{pos[0], pos[1], pos[2]}, d, inv, 0.01f, 100.0f, seqs[l]);
        steps += seqs[l].size();
        any |= seqs[l].size() > 1;
      }
      ++tiles;
      if (!any) {  // (every ray ends at the root: one iteration of the root expansion)
        for (int p = 0; p < 3; ++p) replay(seqs, p, cI, cL, cC, c[p]);
        continue;
      }
      ++busy_tiles;
      for (int l = 0; l < 64; ++l) root_only += seqs[l].size() <= 1;
      for (int p = 0; p < 3; ++p) replay(seqs, p, cI, cL, cC, c[p]);
      // iterations of P0 that run both branches
      std::vector<size_t> pos2(64, 0);
      for (;;) {
        int nI = 0, nL = 0;
        for (int k = 0; k < 64; ++k)
          if (pos2[k] < seqs[k].size()) (seqs[k][pos2[k]] == 'I' ? nI : nL)++, ++pos2[k];
        if (!nI && !nL) break;
        iters0 += 1;
        both += (nI && nL);
      }
    }
  // P1 with lane refill (the ray pump): a wave streams the pixels of 2x1-tile
  // items in queue order (every item of a row of items, frame rows top to
  // bottom) and hands each finished lane the next pixel once >= R lanes are
  // free; stream length = one row of items per wave
  for (int R : {8, 16, 32}) {
    Cost cr;
    for (int ty = 0; ty < H / 8; ++ty) {
      std::vector<std::string> stream;
      for (int tx2 = 0; tx2 < W / 16; ++tx2)
        for (int half = 0; half < 2; ++half)
          for (int l = 0; l < 64; ++l) {
            const int x = (tx2 * 2 + half) * 8 + (l & 7), yo = ty * 8 + (l >> 3), y = H - yo - 1;
            const V3 d = eye(x, y);
            const V3 inv{1.0f / d.x, 1.0f / d.y, 1.0f / d.z};
            std::string sq;
            trace(0, V3{pos[0], pos[1], pos[2]}, d, inv, 0.01f, 100.0f, sq);
            stream.push_back(sq);
          }
      size_t next = 0;
      std::vector<std::string> lane(64);
      std::vector<size_t> at(64, 0);
      std::vector<bool> live(64, false);
      for (;;) {
        int dead = 0;
        for (int k = 0; k < 64; ++k) dead += !live[k];
        if (dead >= R || next == 0)
          for (int k = 0; k < 64 && next < stream.size(); ++k)
            if (!live[k]) { lane[k] = stream[next++]; at[k] = 0; live[k] = !lane[k].empty(); }
        int nI = 0, nL = 0, nlive = 0;
        for (int k = 0; k < 64; ++k)
          if (live[k]) { ++nlive; (lane[k][at[k]] == 'I' ? nI : nL)++; }
        if (!nlive) { if (next >= stream.size()) break; continue; }
        bool runI = nI > 0, runL = nL > 0;
        if (runI && runL) { if (nL * g_k < nI) runL = false; else if (nI * g_k < nL) runI = false; }
        int nM = 0;
        for (int k = 0; k < 64; ++k) nM += live[k] && lane[k][at[k]] == 'M';
        cr.wave_instr += cC + (runI ? cI : 0) + (runL ? (nM ? cL : cL / 2) : 0);
        cr.iters += 1;
        for (int k = 0; k < 64; ++k) {
          if (!live[k]) continue;
          const char c = lane[k][at[k]];
          if ((c == 'I' && runI) || (c != 'I' && runL)) {
            cr.lane_instr += (c == 'I' ? cI : c == 'M' ? cL : cL / 2) + cC;
            if (++at[k] >= lane[k].size()) live[k] = false;
          }
        }
      }
    }
    std::printf("P1 + refill at %2d free lanes: lane util %.3f  wave instr %.4g  iterations %.4g  (x%.3f instr vs P1 per tile; whole frame)\n",
                R, cr.lane_instr / (64.0 * cr.wave_instr), cr.wave_instr, cr.iters, cr.wave_instr / c[1].wave_instr);
  }
  std::printf("tiles %ld (%ld with any ray past the root), steps per ray %.3f\n", tiles, busy_tiles,
              steps / ((double)W * H));
  std::printf("rays of those tiles that end at the root: %.1f %%\n", 100.0 * root_only / (64.0 * busy_tiles));
  std::printf("P0 iterations running both branches: %.1f %%\n", 100.0 * both / iters0);
  const char *name[3] = {"P0 both branches (kernel)", "P1 minority side waits (K)", "P2 inner first"};
  for (int p = 0; p < 3; ++p)
    std::printf("%-28s lane util %.3f  wave instr %.4g  iterations %.4g  (x%.3f instr, x%.3f iters vs P0)\n",
                name[p], c[p].lane_instr / (64.0 * c[p].wave_instr), c[p].wave_instr, c[p].iters,
                c[p].wave_instr / c[0].wave_instr, c[p].iters / c[0].iters);
  return 0;
}
