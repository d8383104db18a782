// felz_weight.h — the Felzenszwalb edge weight of two coloured, oriented points (segmentator.cpp:85-121), shared by the
// mesh kernel (felz.hip) and the point-cloud kernel (felz_points.hip) so that both give the same bits.
// Every multiply/add is rounded separately (fp contract off for the rest of the translation unit), sqrt and division
// are IEEE: the reference is compiled for baseline x86-64, which has no FMA.
#pragma once
#include <math.h>

#include "common.h"

#pragma clang fp contract(off)

namespace usc {

struct V3 { float x, y, z; };
__device__ inline V3 ld3(const float* p, int64_t i) { return V3{p[3 * i], p[3 * i + 1], p[3 * i + 2]}; }

// kOriented: the normals' signs mean something (mesh normals, normals of a file).  normal_dist = 1 - dot, and an edge
// whose far normal leans along the edge (a convex crease) between like colours has its weight squared.
// !kOriented: the sign of each normal is arbitrary (estimated normals), so the convexity test means nothing:
// normal_dist = 1 - |dot| and nothing is squared; the edge direction is not computed.
// p1 == p2 (dd = 0): the direction is NaN, `dot2 > 0` is false, the weight stays the finite product.
template <bool kOriented>
__device__ inline float felz_edge_weight(V3 p1, V3 p2, V3 c1, V3 c2, V3 n1, V3 n2) {
  const float dot = n1.x * n2.x + n1.y * n2.y + n1.z * n2.z;
  const float normal_dist = 1.0f - (kOriented ? dot : fabsf(dot));
  const float color_dist = fabsf(c1.x - c2.x) + fabsf(c1.y - c2.y) + fabsf(c1.z - c2.z);
  float dist = normal_dist * color_dist;
  if (kOriented) {
    float dx = p2.x - p1.x, dy = p2.y - p1.y, dz = p2.z - p1.z;
    const float dd = sqrtf(dx * dx + dy * dy + dz * dz);
    dx /= dd; dy /= dd; dz /= dd;
    const float dot2 = n2.x * dx + n2.y * dy + n2.z * dz;
    if (dot2 > 0 && (double)color_dist < 0.05) dist = dist * dist;   // the reference compares against a double literal
  }
  return dist;
}

}  // namespace usc
