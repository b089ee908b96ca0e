// meshintersect.hpp -- which faces of an indexed mesh cut through each other: self-intersections, and with a group label per face
// the intersections between two meshes.  DESIGN.md "Intersections on the device".
//
// Reference: none in its tree.  The rule is stated once, in integers, by the tensor specification meshing.mesh_intersections, and
// every result here is compared with it bit for bit.  In short:
//
//   * q = llrint(clamp((double(v) - double(origin)) scale, -2^18, 2^18)) per coordinate, the lattice of meshorient.hpp; a face with
//     a vertex id out of range or a non-finite vertex is VOID: it intersects nothing and is counted;
//   * orient(a, b, c, d) = det[b - a; c - a; d - a] in int64 (mi_orient states the bound);
//   * the segment pq PROPERLY CROSSES the triangle abc when orient(a,b,c,p) and orient(a,b,c,q) are non-zero and of opposite sign
//     and orient(p,q,a,b), orient(p,q,b,c), orient(p,q,c,a) are all >= 0 or all <= 0;
//   * two faces f != g INTERSECT when an edge of one properly crosses the other, either way round.  No special case for
//     neighbours: an edge with an end in the other face's plane never crosses it properly, so faces that share a vertex or an
//     edge are reported only when they fold through each other; duplicates, touching contact and coplanar overlap are not
//     intersections; a degenerate face can cut with its edges and cannot be cut;
//   * with `group` and between != 0 only pairs from different groups count.
//
// arah_mesh_intersections, one launch per line:
//
//   k_mi_quant       the quantised soup as float32 [F][3][3] (|q| <= 2^18 is exact in float32; a void face is a point at the origin),
//                    the void flags, vert_hit cleared
//   arah_mesh_index_build   meshdist.hpp's uniform grid over that soup, unchanged
//   k_mi_pairs<0>    one lane per face f: hits[f], the number of partners g > f, vert_hit
//   k_mi_big<0>      one workgroup per face of the index's big list: the same three for that face
//   k_mc_scan        pair_start = the exclusive scan of the partners above, pair_start[F] the total
//   k_mi_tally, k_mi_counts   the vertices hit, the total once more in 64 bits, counts
//   k_mi_pairs<1>, k_mi_big<1>   the partners g > f into f's row of the raw list (in the order they are met)
//   k_mi_sort_short, k_mi_sort_long   rank-count sort of every row into pairs (meshadj.hpp's two kernels' shape), k_mc_pad_words
//
// CANDIDATES.  md_cell_of is monotone in the coordinate and the quantised coordinates are exact, so when the integer boxes of f
// and g overlap, the component-wise maximum m of their lower corners lies in both boxes, and the cell of m -- the pair's HOME
// CELL -- lies in the cell range of either face: both are referenced from it, unless one is on the big list.  A lane walks the at
// most kMdSpan cells of its face's box and tests a pair in its home cell only: exactly once per side, no de-duplication table.
// Floating point locates cells (the same md_cell_of on the same numbers as k_md_bin, and only its monotonicity is used); no
// floating-point arithmetic decides whether two faces intersect, and there are no floating-point atomics.  A face of the big list
// (a box of more than kMdSpan cells: one long triangle in a simplified mesh) is tested by every lane, and has a workgroup of its
// own that strides over all faces.  The marching-cubes body has an empty big list: that path is the tail.
//
// Integer atomics only (add), on sums that do not depend on the order of arrival; hits, the partners above and pair_start have one
// writer each.  No thread waits for another: no spin-wait, no grid-wide barrier; every loop ends by an argument stated at the loop.
// Included by arah_hip.hip after meshdist.hpp.
#pragma once

namespace {

constexpr double kMiLimit = 262144.0;   // 2^18, kMoVolLimit's value: the differences of two coordinates are at most 2^19
constexpr int kMiShort = 32;             // partners of a row one thread still sorts alone (kMaShort's value)
constexpr int kMiBigGrid = 1024;         // workgroups that share the big faces, and the long rows

struct MiAcc {                           // the call's accumulators, cleared by the entry
    unsigned long long total;            // the pairs, in 64 bits: pair_start wraps above 2^31 - 1, this does not
    unsigned long long tested;           // pairs that reached the six tests (the bench's figure, not part of the rule)
    int faces_hit, verts_hit, n_void, unused;
};

struct MiFace {
    int q[3][3];          // corner, axis
    int lo[3], hi[3];     // the integer box
};

__device__ __forceinline__ void mi_load(const float* __restrict__ tris, int f, MiFace& t) {
    const float* v = tris + (size_t)f * 9;
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int a = 0; a < 3; ++a) t.q[k][a] = (int)v[3 * k + a];   // an integer of at most 19 bits: the conversion is exact
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        t.lo[a] = min(t.q[0][a], min(t.q[1][a], t.q[2][a]));
        t.hi[a] = max(t.q[0][a], max(t.q[1][a], t.q[2][a]));
    }
}

// det[b - a; c - a; d - a].  |q| <= 2^18, so every difference is at most 2^19 in magnitude, every product of two at most 2^38, every
// triple product at most 2^57, and the six of them add up to less than 6 * 2^57 < 2^60: exact in int64, whatever the grouping.
__device__ __forceinline__ long long mi_orient(const int* a, const int* b, const int* c, const int* d) {
    const long long ux = b[0] - a[0], uy = b[1] - a[1], uz = b[2] - a[2];
    const long long vx = c[0] - a[0], vy = c[1] - a[1], vz = c[2] - a[2];
    const long long wx = d[0] - a[0], wy = d[1] - a[1], wz = d[2] - a[2];
    return ux * (vy * wz - vz * wy) - uy * (vx * wz - vz * wx) + uz * (vx * wy - vy * wx);
}

// does an edge of e properly cross the triangle t?
__device__ __forceinline__ bool mi_edges_cross(const MiFace& e, const MiFace& t) {
    long long side[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) side[k] = mi_orient(t.q[0], t.q[1], t.q[2], e.q[k]);
    bool cut = false;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int j = (k + 1) % 3;
        if ((side[k] > 0 && side[j] < 0) || (side[k] < 0 && side[j] > 0)) {
            const long long s0 = mi_orient(e.q[k], e.q[j], t.q[0], t.q[1]);
            const long long s1 = mi_orient(e.q[k], e.q[j], t.q[1], t.q[2]);
            const long long s2 = mi_orient(e.q[k], e.q[j], t.q[2], t.q[0]);
            cut = cut || (s0 >= 0 && s1 >= 0 && s2 >= 0) || (s0 <= 0 && s1 <= 0 && s2 <= 0);
        }
    }
    return cut;
}

__device__ __forceinline__ bool mi_intersect(const MiFace& f, const MiFace& g) { return mi_edges_cross(g, f) || mi_edges_cross(f, g); }

__device__ __forceinline__ bool mi_boxes_meet(const MiFace& f, const MiFace& g) {
    return f.lo[0] <= g.hi[0] && g.lo[0] <= f.hi[0] && f.lo[1] <= g.hi[1] && g.lo[1] <= f.hi[1] && f.lo[2] <= g.hi[2] && g.lo[2] <= f.hi[2];
}

// the cell range of a face's box as k_md_bin computes it (the same function on the same numbers); true when the face is on the
// big list
__device__ __forceinline__ bool mi_cells(const MdHeader& H, const MiFace& t, int* c0, int* c1) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        c0[a] = md_cell_of(H, a, (double)t.lo[a]);
        c1[a] = md_cell_of(H, a, (double)t.hi[a]);
    }
    return (long long)(c1[0] - c0[0] + 1) * (c1[1] - c0[1] + 1) * (c1[2] - c0[2] + 1) > kMdSpan;
}

// the sum of v over the wave in every lane.  CONTRACT: all 64 lanes call it together
__device__ __forceinline__ unsigned long long mi_wave_sum(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__device__ __forceinline__ void mi_mark_corners(const int* __restrict__ faces, int f, int n_verts, unsigned char* vert_hit) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int id = faces[3 * (size_t)f + k];
        if ((unsigned)id < (unsigned)n_verts) vert_hit[id] = 1;   // a face that is not void has its ids in range; 1 is all anyone stores
    }
}

__global__ __launch_bounds__(kImeshThreads) void k_mi_quant(const float* __restrict__ verts, int n_verts, const int* __restrict__ faces,
                                                            int n_faces, MoQuant g, float* __restrict__ tris, unsigned char* __restrict__ isvoid,
                                                            unsigned char* __restrict__ vert_hit, MiAcc* acc) {
#pragma clang fp contract(off)
    const long long step = (long long)gridDim.x * blockDim.x, end = ((long long)max(n_verts, n_faces) + 63) & ~63ll;
    // terminates: end - i strictly decreases (step >= 1) and the loop ends when it reaches 0; the count is rounded up to whole waves
    // so that every lane reaches the ballot
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < end; i += step) {
        if (i < n_verts) vert_hit[i] = 0;
        bool bad = false;
        if (i < n_faces) {
            float q[9];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const int id = faces[3 * i + k];
                const bool in = (unsigned)id < (unsigned)n_verts;
                bad = bad || !in;
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    const float x = in ? verts[3 * (size_t)id + a] : 0.0f;
                    const bool fin = isfinite(x);
                    bad = bad || !fin;
                    const double t = ((double)x - (double)g.origin[a]) * g.scale;
                    q[3 * k + a] = fin ? (float)llrint(fmin(fmax(t, -kMiLimit), kMiLimit)) : 0.0f;
                }
            }
#pragma unroll
            for (int k = 0; k < 9; ++k) tris[9 * i + k] = bad ? 0.0f : q[k];
            isvoid[i] = bad ? 1 : 0;
        }
        const unsigned long long n_bad = __ballot(bad);
        if ((threadIdx.x & 63) == 0 && n_bad) atomicAdd(&acc->n_void, (int)__popcll(n_bad));
    }
}

struct MiMesh {
    const float* tris;              // the quantised soup
    const unsigned char* isvoid;
    const unsigned char* group;     // null: every pair counts
    const int* faces;
    int n_faces, n_verts;
};

// is g a partner of f?  f != g, neither void, the group rule, the integer boxes, then the six tests.  `home`: the cell the pair is
// met in, or null for a pair met through the big list, which is met once anyway.
__device__ __forceinline__ bool mi_partner(const MiMesh& m, const MdHeader& H, int f, const MiFace& tf, int g, const int* home,
                                           unsigned long long& tested) {
    if (g == f || (unsigned)g >= (unsigned)m.n_faces || m.isvoid[g]) return false;
    if (m.group && m.group[g] == m.group[f]) return false;
    MiFace tg;
    mi_load(m.tris, g, tg);
    if (!mi_boxes_meet(tf, tg)) return false;
    if (home) {
#pragma unroll
        for (int a = 0; a < 3; ++a)
            if (md_cell_of(H, a, (double)max(tf.lo[a], tg.lo[a])) != home[a]) return false;
    }
    ++tested;
    return mi_intersect(tf, tg);
}

// FILL false: hits[f], above[f] = the partners g > f, vert_hit, the faces hit;  true: the partners g > f into raw[pair_start[f] ..)
// for the rows that start below `cap` (a row has fewer than F entries, and raw has cap + F).  A face of the big list is left to
// k_mi_big.  Launch ceil(F / kImeshThreads) workgroups: one lane per face, whole waves, so that every lane reaches the ballot and
// the shuffles at the end; nothing between them and the top is shared.
template <bool FILL>
__global__ __launch_bounds__(kImeshThreads) void k_mi_pairs(MiMesh m, const MdHeader* __restrict__ hdr, const int* __restrict__ cell_base,
                                                            const int* __restrict__ refs, const int* __restrict__ big, int* __restrict__ hits,
                                                            int* __restrict__ above, unsigned char* vert_hit, const int* __restrict__ pair_start,
                                                            int* __restrict__ raw, long long cap, MiAcc* acc, int want_tested) {
    const long long fl = (long long)blockIdx.x * kImeshThreads + threadIdx.x;
    const int f = (int)fl;
    const MdHeader H = *hdr;
    if (FILL && acc->total > 0x7fffffffull) return;   // pair_start wrapped: nothing is written (the same for every thread)
    bool active = fl < m.n_faces && !m.isvoid[f];
    bool is_big = false;
    int n_hit = 0, n_above = 0;
    unsigned long long tested = 0;
    if (active) {
        MiFace tf;
        mi_load(m.tris, f, tf);
        int c0[3], c1[3];
        is_big = mi_cells(H, tf, c0, c1);
        const long long base = FILL ? (long long)pair_start[f] : 0;
        // the fill pass walks for the faces that have a row to fill: on an embedded mesh for none
        const bool write = FILL && base >= 0 && base < cap && pair_start[f + 1] > pair_start[f];
        if (!is_big && (!FILL || write)) {
            auto visit = [&](int g, const int* home) {
                if (FILL && g < f) return;
                if (!mi_partner(m, H, f, tf, g, home, tested)) return;
                ++n_hit;
                if (g > f) {
                    if (FILL) raw[base + n_above] = g;   // < base + above[f] <= cap + F - 1: the count pass met the same partners
                    ++n_above;
                }
            };
            const int n_big = min(max(H.n_big, 0), m.n_faces);
            for (int k = 0; k < n_big; ++k) visit(big[k], nullptr);   // terminates: n_big - k strictly decreases
            // terminates: at most kMdSpan cells (is_big is false), and cell_base[cell + 1] - k strictly decreases in each
            for (int z = c0[2]; z <= c1[2]; ++z)
                for (int y = c0[1]; y <= c1[1]; ++y)
                    for (int x = c0[0]; x <= c1[0]; ++x) {
                        const int cell = (z * H.n[1] + y) * H.n[0] + x;   // < n_cells: the cells of md_cell_of
                        const int home[3] = {x, y, z};
                        const int e1 = cell_base[cell + 1];
                        for (int k = cell_base[cell]; k < e1; ++k) visit(refs[k], home);
                    }
        }
    }
    if (!FILL) {
        if (fl < m.n_faces && !is_big) {
            hits[f] = n_hit;
            above[f] = n_above;
            if (n_hit > 0) mi_mark_corners(m.faces, f, m.n_verts, vert_hit);
        }
        const unsigned long long hit = __ballot(n_hit > 0);
        if ((threadIdx.x & 63) == 0 && hit) atomicAdd(&acc->faces_hit, (int)__popcll(hit));
    }
    if (want_tested) {   // the same for every thread
        const unsigned long long sum = mi_wave_sum(tested);
        if ((threadIdx.x & 63) == 0 && sum) atomicAdd(&acc->tested, sum);
    }
}

// One workgroup per face of the big list, striding over ALL faces with the box reject; the big faces are shared by the grid.
// FILL false: the workgroup's counts reduced (mesh_prefix's totals), written by thread 0;  true: the partners g > f into f's row of
// raw, the slot by an atomic on a counter of the workgroup (the order inside a row is free: the sort follows).
template <bool FILL>
__global__ __launch_bounds__(kImeshThreads) void k_mi_big(MiMesh m, const MdHeader* __restrict__ hdr, const int* __restrict__ big,
                                                          int* __restrict__ hits, int* __restrict__ above, unsigned char* vert_hit,
                                                          const int* __restrict__ pair_start, int* __restrict__ raw, long long cap, MiAcc* acc,
                                                          int want_tested) {
    __shared__ int wsum[kImeshThreads / 64];
    __shared__ int cursor;
    const MdHeader H = *hdr;
    if (FILL && acc->total > 0x7fffffffull) return;   // the same for every thread
    const int n_big = min(max(H.n_big, 0), m.n_faces);
    // terminates: n_big - k strictly decreases (gridDim.x >= 1).  k, f and the trip counts of the barriers below are the same for
    // every thread of the workgroup
    for (int k = blockIdx.x; k < n_big; k += gridDim.x) {
        const int f = big[k];
        if ((unsigned)f >= (unsigned)m.n_faces || m.isvoid[f]) continue;   // k_md_bin wrote a face id; a void face is a point
        MiFace tf;
        mi_load(m.tris, f, tf);
        const long long base = FILL ? (long long)pair_start[f] : 0;
        const bool write = FILL && base >= 0 && base < cap && pair_start[f + 1] > pair_start[f];   // the same for every thread
        if (FILL) {
            if (threadIdx.x == 0) cursor = 0;
            __syncthreads();
        }
        int n_hit = 0, n_above = 0;
        unsigned long long tested = 0;
        if (!FILL || write) {
            // terminates: n_faces - g strictly decreases
            for (int g = (FILL ? f + 1 : 0) + (int)threadIdx.x; g < m.n_faces; g += kImeshThreads) {
                if (!mi_partner(m, H, f, tf, g, nullptr, tested)) continue;
                ++n_hit;
                if (g > f) {
                    if (FILL) raw[base + atomicAdd(&cursor, 1)] = g;   // < base + above[f] <= cap + F - 1
                    ++n_above;
                }
            }
        }
        if (!FILL) {
            int total_hit, total_above;
            mesh_prefix(n_hit, wsum, total_hit);
            mesh_prefix(n_above, wsum, total_above);
            if (threadIdx.x == 0) {
                hits[f] = total_hit;
                above[f] = total_above;
                if (total_hit > 0) {
                    mi_mark_corners(m.faces, f, m.n_verts, vert_hit);
                    atomicAdd(&acc->faces_hit, 1);
                }
            }
        } else {
            __syncthreads();   // before the next face clears the cursor
        }
        if (want_tested) {
            const unsigned long long sum = mi_wave_sum(tested);
            if ((threadIdx.x & 63) == 0 && sum) atomicAdd(&acc->tested, sum);
        }
    }
}

__global__ __launch_bounds__(kImeshThreads) void k_mi_tally(const unsigned char* __restrict__ vert_hit, int n_verts, const int* __restrict__ above,
                                                            int n_faces, MiAcc* acc) {
    const long long step = (long long)gridDim.x * blockDim.x, end = ((long long)max(n_verts, n_faces) + 63) & ~63ll;
    // terminates: end - i strictly decreases (step >= 1); whole waves, for the ballot and the shuffles
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < end; i += step) {
        const unsigned long long marked = __ballot(i < n_verts && vert_hit[i] != 0);
        const unsigned long long sum = mi_wave_sum(i < n_faces ? (unsigned long long)above[i] : 0ull);
        if ((threadIdx.x & 63) == 0) {
            if (marked) atomicAdd(&acc->verts_hit, (int)__popcll(marked));
            if (sum) atomicAdd(&acc->total, sum);
        }
    }
}

// counts = pairs (-1: more than 2^31 - 1, and then pair_start means nothing and no pair is written), faces hit, vertices hit, void
// faces, pairs written; tested_out (or null)
__global__ void k_mi_counts(const MiAcc* __restrict__ acc, long long cap, int* __restrict__ counts, long long* __restrict__ tested_out,
                            int* __restrict__ pair_total) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const bool over = acc->total > 0x7fffffffull;
    counts[0] = over ? -1 : (int)acc->total;
    counts[1] = acc->faces_hit;
    counts[2] = acc->verts_hit;
    counts[3] = acc->n_void;
    counts[4] = over ? 0 : (int)min((long long)acc->total, cap);
    if (over) *pair_total = -1;
    if (tested_out) *tested_out = (long long)acc->tested;
}

// Rank-count sort of f's raw row into pairs (ma_rank_sort's rule; the partners of a face are distinct): the rows that start below
// cap, and of those the entries that land below it.
__device__ __forceinline__ void mi_sort_row(const int* __restrict__ pair_start, const int* __restrict__ raw, int* __restrict__ pairs,
                                            long long cap, int f, bool want_long, int tid, int nthreads) {
    const long long s = pair_start[f];
    const int n = pair_start[f + 1] - pair_start[f];
    if (s < 0 || s >= cap || n <= 0 || (n > kMiShort) != want_long) return;
    // terminates: n - i strictly decreases (nthreads >= 1); the inner loop runs n times
    for (int i = tid; i < n; i += nthreads) {
        const int x = raw[s + i];
        int rank = 0;
        for (int j = 0; j < n; ++j) rank += raw[s + j] < x ? 1 : 0;
        if (s + rank < cap) {
            pairs[2 * (s + rank) + 0] = f;
            pairs[2 * (s + rank) + 1] = x;
        }
    }
}

__global__ __launch_bounds__(kImeshThreads) void k_mi_sort_short(const int* __restrict__ pair_start, int n_faces, const int* __restrict__ raw,
                                                                 int* __restrict__ pairs, long long cap, const MiAcc* __restrict__ acc) {
    if (acc->total > 0x7fffffffull) return;
    const long long step = (long long)gridDim.x * blockDim.x;
    // terminates: n_faces - f strictly decreases (step >= 1) and the loop ends when it reaches 0
    for (long long f = (long long)blockIdx.x * blockDim.x + threadIdx.x; f < n_faces; f += step)
        mi_sort_row(pair_start, raw, pairs, cap, (int)f, false, 0, 1);
}

__global__ __launch_bounds__(kImeshThreads) void k_mi_sort_long(const int* __restrict__ pair_start, int n_faces, const int* __restrict__ raw,
                                                                int* __restrict__ pairs, long long cap, const MiAcc* __restrict__ acc) {
    if (acc->total > 0x7fffffffull) return;
    // terminates: n_faces - f strictly decreases (gridDim.x >= 1).  f and the row are the same for every thread of the workgroup;
    // nothing is shared between its threads but the read-only raw row
    for (long long f = blockIdx.x; f < n_faces; f += gridDim.x) mi_sort_row(pair_start, raw, pairs, cap, (int)f, true, (int)threadIdx.x, kImeshThreads);
}

}  // namespace
