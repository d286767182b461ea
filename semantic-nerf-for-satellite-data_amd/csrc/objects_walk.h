// The lock-free union of snerf_objects_link (include/snerf_objects.h): find and unite over a `parent` array, templated on a small
// memory policy so that the SAME loops run in the kernel (csrc/objects.hip: relaxed agent-scope device atomics) and in a host
// program under ThreadSanitizer (csrc/objects_walk_main.cpp: std::atomic<int>).  No HIP in here.
//
// A policy M gives   int load(int cell)               a relaxed atomic load of parent[cell]
//                    int fetch_min(int cell, int v)   atomic parent[cell] = min(parent[cell], v), returning the old word.
//
// Invariant: a link points to a LOWER index of the same component (init: parent[c] = c; fetch_min only lowers).  Every step of both
// loops then strictly lowers a non-negative integer.  The loops enforce what they rely on: a loaded word that is negative or above
// its cell ends the walk and is reported (the caller counts it), so no memory content can make a walk run on.  A stale load is
// harmless: it is an older ancestor.
#pragma once

#if defined(__HIPCC__)
#define SNERF_WALK_FN __host__ __device__ __forceinline__
#else
#define SNERF_WALK_FN inline
#endif

namespace snerf {

// the root of `a`, or -1 when the guard tripped
template <typename M>
SNERF_WALK_FN int walk_find(M& m, int a) {
  for (;;) {
    const int p = m.load(a);
    if (p == a) return a;
    if (p < 0 || p > a) return -1;
    a = p;                                                   // p < a
  }
}

// unite the components of a and b; returns the number of guard trips (0 or 1: a trip ends the call)
template <typename M>
SNERF_WALK_FN int walk_unite(M& m, int a, int b) {
  for (;;) {
    a = walk_find(m, a);
    b = walk_find(m, b);
    if (a < 0 || b < 0) return 1;
    if (a == b) return 0;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = m.fetch_min(a, b);                       // hook the higher root under the lower one
    if (old == a) return 0;                                  // it was still a root: done
    if (old < 0 || old > a) return 1;
    a = old;                                                 // someone hooked it first, under old < a: go on from there
  }
}

}  // namespace snerf
