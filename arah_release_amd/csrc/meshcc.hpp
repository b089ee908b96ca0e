// meshcc.hpp -- connected components of an indexed mesh and the order-preserving selection of some of them, on the device.
//
// Reference: none.  The reference writes the mesh skimage extracts as it comes (utils/sdf_meshing.py:95-114); a SIREN trained on
// captures leaves detached pockets and floaters in it, and every score and per-vertex attribute is then computed on them too.
// Connectivity here is by SHARED VERTEX IDS of an indexed mesh (mcubes.hpp, second half): two vertices are connected when a face
// names both; positions play no part.  Integers only, so the result is unique and is compared bit for bit with the tensor
// specification (meshing.mesh_components / meshing.mesh_select).
//
// arah_mesh_components, one launch per line:
//
//   k_cc_init      parent[v] = v, the two size tables zeroed
//   k_cc_hook      one thread per face: union(a, b), union(a, c) by integer atomicMin on parent under the invariant
//                  parent[x] <= x (cc_union: hook the ends of the two chains, then compress the chains by the same atomic step).
//                  A face with an id outside [0, V) is skipped
//   k_cc_flatten   root[v] = the end of v's parent chain; read-only on parent (the launch boundary made it final), a separate
//                  array is written.  The root of a component is its smallest vertex id
//   k_cc_compact<kCcRoots, false>, k_mc_scan, k_cc_compact<kCcRoots, true>
//                  the count / scan / fill of meshcommon.hpp over the marks root[v] == v: dense[r] = the number of roots below r,
//                  so components are numbered in ascending order of their smallest vertex id; the total is C
//   k_cc_label     labels[v] = dense[root[v]], comp_verts[label] += 1
//   k_cc_faces     comp_faces[label of a valid face] += 1, counts[1] += 1
//   k_cc_largest   max over c < C of the packed word (comp_faces[c] << 32) | (2^32 - 1 - c): most faces, ties to the lowest id
//   k_cc_finish    counts[2] from that word
//
// arah_mesh_select: k_cc_compact<kCcVerts> (count, k_mc_scan, fill: vert_map, vert_src), k_cc_compact<kCcFaces> (count,
// k_mc_scan, fill: faces_out, face_src), k_mc_pad_words for the rows between the counts and the arrays' lengths.
//
// Every atomic is an integer atomicMin / atomicAdd / atomicMax: minima, sums and maxima of integers do not depend on the order
// of arrival.  No thread ever waits for another lane, wave or workgroup: there is no spin-wait and no grid-wide barrier, every
// loop ends by an argument local to its own thread (or, for cc_add_one of meshcommon.hpp, its own wave in lockstep), stated at
// the loop.  The constants, mesh_compact, k_mc_scan, k_mc_pad_words and cc_add_one are meshcommon.hpp's.
#pragma once

// Why hooking is right.  Let G be the graph of the links in place (x, parent[x]), the pairs (a, b) that threads inside cc_union
// still have to join, and the edges of the faces not yet visited.  G starts as the mesh's own vertex graph, and no step ever
// separates two vertices G connects:
//   * atomicMin(&parent[hi], lo) returning old: the link (hi, old) and the pair (hi, lo) become the link (hi, min(old, lo)) and
//     the pair (old, lo) -- hi, old and lo stay together (old == hi: the pair is simply done);
//   * a walk reaches a vertex over values parent[] held at SOME time: each such link joined two vertices G connected then, hence
//     connects now; so a pair made of a vertex and the end of its walk adds nothing to G, and may be joined like any other.
// At the end of the launch no pair and no face is left: G is the forest of parent[], a tree per component, and since
// parent[x] <= x the root of a tree is its smallest vertex.  parent[x] is written by atomicMin only.

// Follow x's parent chain with plain loads.  They may be stale, so the result is only a STARTING POINT for cc_join.
__device__ __forceinline__ int cc_walk(const int* parent, int x) {
    int p = parent[x];
    // terminates: x strictly decreases (parent[x] <= x, with equality only where the walk stops) and is bounded below by 0
    while (p != x) {
        x = p;
        p = parent[x];
    }
    return x;
}

// Join a and b, two vertices G connects or is to connect, by atomics alone.  The only decision is taken on what atomicMin
// RETURNS: `old == hi` means hi was a root at the instant of the atomic and now hangs below lo -- done.  Otherwise hi already
// hung below old < hi; whether that link survived (old <= lo) or was displaced by lo (lo < old), old and lo still have to meet,
// and this thread sees to it.  Every vertex the loop visits ends up hanging below lo or lower: joining a vertex to a vertex
// further down its own tree is PATH COMPRESSION, by the same step and under the same invariant.
__device__ __forceinline__ void cc_join(int* parent, int a, int b) {
    // terminates: max(a, b) strictly decreases from one round to the next (old < hi and lo < hi) and is bounded below by 0; a
    // round never waits for another thread
    while (a != b) {
        const int hi = max(a, b), lo = min(a, b);
        const int old = atomicMin(&parent[hi], lo);
        if (old == hi) return;
        a = old;
        b = lo;
    }
}

// One edge (a, b) of a face: read-only walks find where the two chains end at the moment (starting points), cc_join hooks the
// two ends, and then a and b themselves are joined to the lower end, which re-hangs every vertex of their two chains there.
// Without that last step the cost is set by the depth of the chains, and that by the order in which faces arrive: replayed
// one face after the other, the 9 702-vertex level set of a sphere at 65^3 in DESCENDING face order builds chains 7 561 deep
// (4.5 M walk steps here, 3.8e7 loads in k_cc_flatten); with it 67 deep (8.4e4 and 2.6e5), for about ten atomics per face.
__device__ __forceinline__ void cc_union(int* parent, int a, int b) {
    const int ra = cc_walk(parent, a), rb = cc_walk(parent, b);
    cc_join(parent, ra, rb);
    const int lo = min(ra, rb);
    cc_join(parent, a, lo);
    cc_join(parent, b, lo);
}

__device__ __forceinline__ bool cc_face_ok(const int* __restrict__ faces, long long f, int n_verts, int id[3]) {
    id[0] = faces[3 * f + 0];
    id[1] = faces[3 * f + 1];
    id[2] = faces[3 * f + 2];
    return (unsigned)id[0] < (unsigned)n_verts && (unsigned)id[1] < (unsigned)n_verts && (unsigned)id[2] < (unsigned)n_verts;
}

__global__ __launch_bounds__(kImeshThreads) void k_cc_init(int* __restrict__ parent, int* __restrict__ comp_verts,
                                                           int* __restrict__ comp_faces, int n_verts, int* __restrict__ counts,
                                                           unsigned long long* __restrict__ best) {
    const long long step = (long long)gridDim.x * blockDim.x;
    // terminates: n_verts - v strictly decreases (step >= 1) and the loop ends when it reaches 0
    for (long long v = (long long)blockIdx.x * blockDim.x + threadIdx.x; v < n_verts; v += step) {
        parent[v] = (int)v;
        comp_verts[v] = 0;
        comp_faces[v] = 0;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        counts[0] = 0;
        counts[1] = 0;
        counts[2] = -1;
        *best = 0ull;
    }
}

__global__ __launch_bounds__(kImeshThreads) void k_cc_hook(const int* __restrict__ faces, int n_faces, int n_verts, int* parent) {
    const long long step = (long long)gridDim.x * blockDim.x;
    // terminates: n_faces - f strictly decreases (step >= 1) and the loop ends when it reaches 0
    for (long long f = (long long)blockIdx.x * blockDim.x + threadIdx.x; f < n_faces; f += step) {
        int id[3];
        if (!cc_face_ok(faces, f, n_verts, id)) continue;
        cc_union(parent, id[0], id[1]);
        cc_union(parent, id[0], id[2]);
    }
}

__global__ __launch_bounds__(kImeshThreads) void k_cc_flatten(const int* __restrict__ parent, int n_verts, int* __restrict__ root) {
    const long long step = (long long)gridDim.x * blockDim.x;
    // terminates: n_verts - v strictly decreases (step >= 1) and the loop ends when it reaches 0
    for (long long v = (long long)blockIdx.x * blockDim.x + threadIdx.x; v < n_verts; v += step) {
        int x = (int)v, p = parent[x];
        // terminates: x strictly decreases (parent[x] < x off a root) and is bounded below by 0
        while (p != x) {
            x = p;
            p = parent[x];
        }
        root[v] = x;
    }
}

// mesh_compact (meshcommon.hpp) over n elements: FILL = false counts the marks of every chunk, k_mc_scan numbers the chunks,
// FILL = true gives a marked element its id.
// WHAT                 mark of element i                                              fill
//   kCcRoots           a[i] == i  (a = root)                                          o0[i] = id  (dense, roots only)
//   kCcVerts           b[a[i]] != 0  (a = labels, b = keep; a label outside [0, V)    o0[i] = id or -1 (vert_map), o1[id] = i
//                      marks nothing)                                                 (vert_src)
//   kCcFaces           face i is valid and a[] >= 0 at its three ids (a = vert_map)   o0[id][3] = a[ids] (faces_out), o1[id] = i
//                                                                                     (face_src)
enum { kCcRoots = 0, kCcVerts = 1, kCcFaces = 2 };

struct CcCorners {
    int id[3];   // kCcFaces: the new ids of the face's three corners
};

template <int WHAT, bool FILL>
__global__ __launch_bounds__(kImeshThreads) void k_cc_compact(const int* __restrict__ faces, const int* __restrict__ a,
                                                              const int* __restrict__ b, int n, int n_verts,
                                                              int* __restrict__ blk_count, const int* __restrict__ blk_base,
                                                              int* __restrict__ o0, int* __restrict__ o1) {
    mesh_compact<FILL, CcCorners>(
        n, blk_count, blk_base,
        [&](long long i, CcCorners& c) {
            if constexpr (WHAT == kCcRoots) return a[i] == (int)i;
            if constexpr (WHAT == kCcVerts) {
                const int l = a[i];
                return (unsigned)l < (unsigned)n_verts && b[l] != 0;
            }
            if constexpr (WHAT == kCcFaces) {
                if (!cc_face_ok(faces, i, n_verts, c.id)) return false;
                c.id[0] = a[c.id[0]];
                c.id[1] = a[c.id[1]];
                c.id[2] = a[c.id[2]];
                return c.id[0] >= 0 && c.id[1] >= 0 && c.id[2] >= 0;
            }
        },
        [&](long long i, bool ok, bool mark, int at, const CcCorners& c) {
            if constexpr (WHAT == kCcRoots) {
                if (mark) o0[i] = at;
            }
            if constexpr (WHAT == kCcVerts) {
                if (ok) o0[i] = mark ? at : -1;
                if (mark) o1[at] = (int)i;
            }
            if constexpr (WHAT == kCcFaces) {
                if (mark) {
                    o0[3 * (long long)at + 0] = c.id[0];
                    o0[3 * (long long)at + 1] = c.id[1];
                    o0[3 * (long long)at + 2] = c.id[2];
                    o1[at] = (int)i;
                }
            }
        });
}

// The element-wise walks below round the element count up to whole waves, so that every lane of a wave reaches cc_add_one
// and the shuffles together; lanes beyond the end carry active = false.
__global__ __launch_bounds__(kImeshThreads) void k_cc_label(const int* __restrict__ root, const int* __restrict__ dense, int n_verts,
                                                            int* __restrict__ labels, int* comp_verts) {
    const long long step = (long long)gridDim.x * blockDim.x, end = ((long long)n_verts + 63) & ~63ll;
    // terminates: end - v strictly decreases (step >= 1) and the loop ends when it reaches 0
    for (long long v = (long long)blockIdx.x * blockDim.x + threadIdx.x; v < end; v += step) {
        const bool ok = v < n_verts;
        const int c = ok ? dense[root[v]] : 0;
        if (ok) labels[v] = c;
        cc_add_one(comp_verts, c, ok);
    }
}

__global__ __launch_bounds__(kImeshThreads) void k_cc_faces(const int* __restrict__ faces, int n_faces, int n_verts,
                                                            const int* __restrict__ labels, int* comp_faces, int* counts) {
    const long long step = (long long)gridDim.x * blockDim.x, end = ((long long)n_faces + 63) & ~63ll;
    const int lane = threadIdx.x & 63;
    // terminates: end - f strictly decreases (step >= 1) and the loop ends when it reaches 0
    for (long long f = (long long)blockIdx.x * blockDim.x + threadIdx.x; f < end; f += step) {
        int id[3];
        const bool ok = f < n_faces && cc_face_ok(faces, f, n_verts, id);
        const int c = ok ? labels[id[0]] : 0;
        cc_add_one(comp_faces, c, ok);
        const unsigned long long valid = __ballot(ok);
        if (lane == 0 && valid) atomicAdd(&counts[1], (int)__popcll(valid));
    }
}

__global__ __launch_bounds__(kImeshThreads) void k_cc_largest(const int* __restrict__ comp_faces, const int* __restrict__ counts,
                                                              unsigned long long* best) {
    const int n_comp = counts[0];
    const long long step = (long long)gridDim.x * blockDim.x, end = ((long long)n_comp + 63) & ~63ll;
    const int lane = threadIdx.x & 63;
    // terminates: end - c strictly decreases (step >= 1) and the loop ends when it reaches 0
    for (long long c = (long long)blockIdx.x * blockDim.x + threadIdx.x; c < end; c += step) {
        // more faces win, then the LOWER id; a word of a component is never 0 (c < 2^31), 0 is "no component"
        unsigned long long key = c < n_comp ? ((unsigned long long)(unsigned)comp_faces[c] << 32) | (0xFFFFFFFFull - (unsigned long long)c) : 0ull;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long other = __shfl_xor(key, o);
            key = other > key ? other : key;
        }
        if (lane == 0) atomicMax(best, key);
    }
}

__global__ void k_cc_finish(const unsigned long long* __restrict__ best, int* __restrict__ counts) {
    if (blockIdx.x == 0 && threadIdx.x == 0) counts[2] = counts[0] > 0 ? (int)(0xFFFFFFFFull - (*best & 0xFFFFFFFFull)) : -1;
}

// the first n <= 3 counts of an empty call: {components, valid faces, largest} / {kept vertices, kept faces}
__global__ void k_cc_set_counts(int* __restrict__ counts, int c0, int c1, int c2, int n) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        if (n > 0) counts[0] = c0;
        if (n > 1) counts[1] = c1;
        if (n > 2) counts[2] = c2;
    }
}
