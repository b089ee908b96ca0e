// meshcollapse.hpp -- one round of edge-collapse decimation of an indexed mesh, on the device.
//
// Reference: none (see meshsimp.hpp).  Vertex clustering (meshsimp.hpp) welds whatever falls into one cell, so its result is in
// general no surface any more.  Here an edge {u, v} collapses to one vertex only when the surface stays one: both ends interior
// to a consistently oriented two-manifold neighbourhood, the link condition, no face turned over.  The new vertex sits at the
// minimiser of the plane quadric of the faces around the edge (meshquadric.hpp's term, tree and solve, about the midpoint), and
// the quadric's value there is the edge's cost.  The rule is meshing.mesh_collapse_round, float64 with every operation rounded
// on its own and a summation order that is part of the rule; every decision is taken on integers or on the bits of a rounded
// number, so the result is compared with it bit for bit.
//
// MANY EDGES PER ROUND, INDEPENDENT OF THE ORDER OF ARRIVAL.  key(e) = (bits(cost32) << 32) | edge id is unique.  m1[x] = the
// least key of the candidate edges at x, m2[x] = the least of m1 over x and its neighbours, and an edge is selected when m2[u] =
// m2[v] = key(e).  A selected edge is therefore the least of ALL candidate edges at the vertices of N[u] and N[v] (the closed
// neighbourhoods).  Let e' = {u', v'} be selected too and let u' lie in N[u]: then u lies in N[u'], so key(e') = m2[u'] <=
// m1[u] <= key(e) and key(e) = m2[u] <= m1[u'] <= key(e'): the keys are equal and e' = e.  Hence no end of another selected edge
// is u, v or a neighbour of either; the faces two selected edges touch are disjoint; and no vertex the link test or the flip test
// of e looked at (all of them neighbours of u or v) moves or merges in the same round.  Minima over integers do not depend on
// the order of arrival.
//
// arah_mesh_collapse_round, one launch per line (after arah_mesh_adjacency's own, called on the current faces):
//
//   k_mx_pin           one thread per vertex: pinned (non-finite, no neighbour, an entry that is not one face each way); the owner
//                      of every neighbour entry; m1 = empty, merge_to = vsrc = the vertex itself, move_edge = -1; counts cleared
//   k_mx_edge          one LANE per neighbour entry with nbr > owner: link test by a merge of the two neighbour segments, the two
//                      third vertices by a merge of the two face segments, the tree over the ten numbers of the faces around the
//                      edge (the same merge feeds mq_lane_tree, ascending face id), solve, cost, flip test by the merge once
//                      more; writes position, key and reason; atomicMin of the key into m1 of both ends; the reasons counted
//   k_mx_m2            one thread per vertex: m2 = the least of m1 over itself and its sorted neighbours (a gather)
//   k_mx_select<false>, k_mc_scan, k_mx_select<true>
//                      count / scan / fill over the entries with the mark "selected": the first `need` in ascending edge id are
//                      applied -- merge_to[v] = u, move_edge[u] = the edge, vsrc[u] = the nearer of u and v
//   k_mx_verts<false>, k_mc_scan, k_mx_verts<true>
//                      the vertices that were not merged away, in order: new ids, positions, vert_src; rows past the count zeroed
//   k_mx_faces<false>, k_mc_scan, k_mx_faces<true>
//                      the faces that do not name both ends of an applied edge, in order and orientation, renamed; face_src
//   k_mx_finish        counts[3] = min(selected, need)
//
// Integer atomics only (min, add).  No thread waits for another: no spin-wait, no grid-wide barrier; every loop ends by an
// argument of its own, stated at the loop.  MeshAdj is meshadj.hpp's; the owner fill, the entry walk, the merge (MaMerge) and the
// float64 helpers (ma_d2, ma_dot, ma_cross) are meshedge.hpp's.
//
// arah_mesh_collapse_round_bounded runs the same launches with `bounded` set, for the isotropic remesher (meshflip.hpp tells the
// rest): k_mx_edge then refuses, BEFORE every other test, an edge whose squared length in double is not below short_len2 (reason
// 7), and, after the flip test and inside its merge, an edge with a ring vertex -- a corner other than u, v of a face that names
// one of them -- farther than long_len2 (squared) from the new position (reason 8); k_mx_pin clears fourteen counts instead of
// twelve, and the two reasons are counted at 12 and 13.  Without `bounded` neither test runs and no count beyond the twelfth is
// touched: arah_mesh_collapse_round is what it was.
//
// NOT MEASURED AGAINST AN ALTERNATIVE: one lane per edge (its tree keeps 6 x 10 doubles of partial sums in registers, which
// bounds the occupancy, and the lanes of a wave diverge on the reason and on the segment lengths; a wave per edge with the ten
// columns spread over lanes is the alternative); streaming the merge of the two face segments three times from the cache
// instead of keeping the up to 32 face ids in LDS (32 KiB per workgroup) or in scratch; the owner array (meshedge.hpp tells
// that one); kMqShort = 32 as the bound on the faces around an edge, which also caps the valence decimation can grow
// -- a choice.
#pragma once

constexpr unsigned long long kMxEmpty = ~0ull;   // no key: a key's upper half is the bits of a non-negative finite float
constexpr int kMxNoEdge = 255;                   // edge_reason of an entry that names no edge
constexpr int kMxCounts = 12;                    // n_verts, n_faces, selected, applied, candidates, six reasons, fallbacks
constexpr int kMxBoundedCounts = 14;             // arah_mesh_collapse_round_bounded: and the reasons 7 (not short) and 8 (too long)

__global__ __launch_bounds__(kImeshThreads) void k_mx_pin(const float* __restrict__ verts, MeshAdj adj,
                                                          unsigned char* __restrict__ pinned, int* __restrict__ owner,
                                                          unsigned long long* __restrict__ m1, int* __restrict__ merge_to,
                                                          int* __restrict__ move_edge, int* __restrict__ vsrc, int* __restrict__ counts,
                                                          int n_counts) {
    if (blockIdx.x == 0 && threadIdx.x < n_counts) counts[threadIdx.x] = 0;
    const long long step = (long long)gridDim.x * blockDim.x;
    // terminates: n_verts - v strictly decreases (step >= 1) and the loop ends when it reaches 0
    for (long long v = (long long)blockIdx.x * blockDim.x + threadIdx.x; v < adj.n_verts; v += step) {
        const int first = adj.nbr_start[v], last = adj.nbr_start[v + 1];
        bool pin = first == last || !ma_finite(verts, v);
        ma_fill_owner(adj, v, owner);
        for (int i = first; i < last; ++i) pin = pin || adj.nbr_out[i] != 1 || adj.nbr_in[i] != 1;   // terminates: last - i decreases
        pinned[v] = pin ? 1 : 0;
        m1[v] = kMxEmpty;
        merge_to[v] = (int)v;
        move_edge[v] = -1;
        vsrc[v] = (int)v;
    }
}

__global__ __launch_bounds__(kImeshThreads) void k_mx_edge(const float* __restrict__ verts, const int* __restrict__ faces, MeshAdj adj,
                                                           int n_entries_cap, const unsigned char* __restrict__ pinned,
                                                           const int* __restrict__ owner,
                                                           double reg, float max_cost, int bounded, double short_len2,
                                                           double long_len2, float* __restrict__ edge_pos,
                                                           unsigned long long* __restrict__ edge_key, unsigned char* __restrict__ edge_reason,
                                                           unsigned long long* m1, int* counts) {
#pragma clang fp contract(off)
    ma_entry_walk(adj, owner, n_entries_cap, [&](long long i, bool is_edge, int u, int v) {
#pragma clang fp contract(off)
        int reason = 0;
        bool fell = false;
        float pos[3] = {0.f, 0.f, 0.f};
        unsigned long long key = kMxEmpty;
        if (is_edge) {
            // the bounded entry's first test; not a number: refused
            if (bounded && !(ma_d2(verts + 3 * (size_t)u, verts + 3 * (size_t)v) < short_len2)) {
                reason = 7;
            } else if (pinned[u] || pinned[v]) {
                reason = 1;
            } else {
                bool both;
                int common = 0, shared = 0, third[2] = {-1, -1};
                MaMerge w = ma_merge(adj.nbr, adj.nbr_start, u, v);
                while (ma_more(w)) {   // terminates: every call consumes an element of the two segments
                    ma_next(w, both);
                    common += both ? 1 : 0;
                }
                w = ma_merge(adj.vf, adj.vf_start, u, v);
                while (ma_more(w)) {   // terminates: as above
                    const int f = ma_next(w, both);
                    if (both) {   // a valid face of this mesh: its ids lie in [0, V) and two of them are u and v
                        if (shared < 2) third[shared] = faces[3 * (size_t)f + 0] + faces[3 * (size_t)f + 1] + faces[3 * (size_t)f + 2] - u - v;
                        ++shared;
                    }
                }
                // the faces around the edge: both ends are free, so exactly two faces name both
                const int n = (adj.vf_start[u + 1] - adj.vf_start[u]) + (adj.vf_start[v + 1] - adj.vf_start[v]) - 2;
                const int a = third[0], b = third[1];
                if (shared != 2 || a == b || common != 2 || adj.nbr_start[a + 1] - adj.nbr_start[a] < 4 ||
                    adj.nbr_start[b + 1] - adj.nbr_start[b] < 4) {
                    reason = 2;
                } else if (n > kMqShort) {
                    reason = 3;
                } else {
                    double pu[3], pv[3], m[3], cell = 0.0;
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        pu[c] = (double)verts[3 * (size_t)u + c];
                        pv[c] = (double)verts[3 * (size_t)v + c];
                        m[c] = (pu[c] + pv[c]) * 0.5;
                        cell = fmax(cell, fabs(pu[c] - pv[c]));
                    }
                    double q[10];
                    w = ma_merge(adj.vf, adj.vf_start, u, v);
                    // n calls, each consumes at least one of the n + 2 elements of the two segments and the two shared faces
                    // consume two: the merge holds exactly n values
                    mq_lane_tree<10>(n, [&](int, double x[10]) { mq_term<10>(verts, faces, (long long)ma_next(w, both), m, x); }, q);
                    double y[3] = {0.0, 0.0, 0.0};
                    fell = !mq_solve_offset(q, cell, reg, y);
#pragma unroll
                    for (int c = 0; c < 3; ++c) pos[c] = fell ? (float)m[c] : (float)(m[c] + y[c]);
                    const double Ay0 = (q[0] * y[0] + q[1] * y[1]) + q[2] * y[2];
                    const double Ay1 = (q[1] * y[0] + q[3] * y[1]) + q[4] * y[2];
                    const double Ay2 = (q[2] * y[0] + q[4] * y[1]) + q[5] * y[2];
                    const double raw = (((y[0] * Ay0 + y[1] * Ay1) + y[2] * Ay2) + 2.0 * ((q[6] * y[0] + q[7] * y[1]) + q[8] * y[2])) + q[9];
                    const float c32 = (float)raw;
                    const float cost32 = raw > 0.0 ? c32 : 0.f;
                    if (!isfinite(c32)) {
                        reason = 4;
                    } else if (cost32 > max_cost) {
                        reason = 5;
                    } else {
                        const double pn[3] = {(double)pos[0], (double)pos[1], (double)pos[2]};
                        bool flipped = false, far = false;
                        w = ma_merge(adj.vf, adj.vf_start, u, v);
                        while (ma_more(w)) {   // terminates: as above
                            const int f = ma_next(w, both);
                            if (both) continue;
                            double p[3][3], n0[3], n1[3];
                            int moves = 0;
#pragma unroll
                            for (int c = 0; c < 3; ++c) {
                                const int id = faces[3 * (size_t)f + c];
                                moves = (id == u || id == v) ? c : moves;
#pragma unroll
                                for (int x = 0; x < 3; ++x) p[c][x] = (double)verts[3 * (size_t)id + x];
                                if (bounded && id != u && id != v) {   // a vertex of the ring: how far from the new position
                                    const double dx = p[c][0] - pn[0], dy = p[c][1] - pn[1], dz = p[c][2] - pn[2];
                                    far = far || (dx * dx + dy * dy) + dz * dz > long_len2;
                                }
                            }
                            ma_cross(p[0], p[1], p[2], n0);
#pragma unroll
                            for (int c = 0; c < 3; ++c)
#pragma unroll
                                for (int x = 0; x < 3; ++x) p[c][x] = c == moves ? pn[x] : p[c][x];
                            ma_cross(p[0], p[1], p[2], n1);
                            flipped = flipped || !(ma_dot(n0, n1) > 0.0);
                        }
                        if (flipped) {
                            reason = 6;
                        } else if (far) {
                            reason = 8;
                        } else {   // cost32 >= +0 and finite: its bits order like the number
                            key = ((unsigned long long)__float_as_uint(cost32) << 32) | (unsigned long long)i;
                            atomicMin(&m1[u], key);
                            atomicMin(&m1[v], key);
                        }
                    }
                }
            }
        }
        if (i < n_entries_cap) {
            edge_pos[3 * i + 0] = pos[0];
            edge_pos[3 * i + 1] = pos[1];
            edge_pos[3 * i + 2] = pos[2];
            edge_key[i] = key;
            edge_reason[i] = (unsigned char)(is_edge ? reason : kMxNoEdge);
        }
        cc_add_one(counts, reason <= 6 ? 4 + reason : 5 + reason, is_edge);   // reason <= 6: counts[4 .. 10]; 7, 8 (bounded): 12, 13
        cc_add_one(counts + 11, 0, fell);
    });
}

__global__ __launch_bounds__(kImeshThreads) void k_mx_m2(int n_verts, const int* __restrict__ nbr_start, const int* __restrict__ nbr,
                                                         const unsigned long long* __restrict__ m1, unsigned long long* __restrict__ m2) {
    const long long step = (long long)gridDim.x * blockDim.x;
    // terminates: n_verts - v strictly decreases (step >= 1) and the loop ends when it reaches 0
    for (long long v = (long long)blockIdx.x * blockDim.x + threadIdx.x; v < n_verts; v += step) {
        unsigned long long least = m1[v];
        const int last = nbr_start[v + 1];
        for (int i = nbr_start[v]; i < last; ++i) least = min(least, m1[nbr[i]]);   // terminates: last - i strictly decreases
        m2[v] = least;
    }
}

// the selected edges in ascending id; FILL: the first `need` of them are applied
template <bool FILL>
__global__ __launch_bounds__(kImeshThreads) void k_mx_select(const float* __restrict__ verts, MeshAdj adj, int n_entries_cap,
                                                             const int* __restrict__ owner, const float* __restrict__ edge_pos,
                                                             const unsigned long long* __restrict__ edge_key,
                                                             const unsigned long long* __restrict__ m2, int need,
                                                             int* __restrict__ blk_count, const int* __restrict__ blk_base,
                                                             int* __restrict__ merge_to, int* __restrict__ move_edge, int* __restrict__ vsrc) {
    const int n_entries = adj.nbr_start[adj.n_verts];
    mesh_compact<FILL, MeshNoState>(
        n_entries_cap, blk_count, blk_base,
        [&](long long i, MeshNoState&) {
            if (i >= n_entries) return false;
            const unsigned long long key = edge_key[i];
            return key != kMxEmpty && m2[owner[i]] == key && m2[adj.nbr[i]] == key;
        },
        [&](long long i, bool ok, bool mark, int at, const MeshNoState&) {
            if (mark && at < need) {   // selected edges share no end: every row below is written by one edge at most
                const int u = owner[i], v = adj.nbr[i];
                const float pos[3] = {edge_pos[3 * i + 0], edge_pos[3 * i + 1], edge_pos[3 * i + 2]};
                merge_to[v] = u;
                move_edge[u] = (int)i;
                // the nearer end by float32 of the squared distances, which are evaluated in double
                vsrc[u] = (float)ma_d2(verts + 3 * (size_t)v, pos) < (float)ma_d2(verts + 3 * (size_t)u, pos) ? v : u;
            }
        });
}

// the vertices that stay, in order
template <bool FILL>
__global__ __launch_bounds__(kImeshThreads) void k_mx_verts(const float* __restrict__ verts, int n_verts, const int* __restrict__ merge_to,
                                                            const int* __restrict__ move_edge, const int* __restrict__ vsrc,
                                                            const float* __restrict__ edge_pos, int* __restrict__ blk_count,
                                                            const int* __restrict__ blk_base, const int* __restrict__ counts,
                                                            int* __restrict__ new_id, float* __restrict__ verts_out, int* __restrict__ vert_src) {
    const int kept = FILL ? counts[0] : 0;
    mesh_compact<FILL, MeshNoState>(
        n_verts, blk_count, blk_base, [&](long long v, MeshNoState&) { return merge_to[v] == (int)v; },
        [&](long long v, bool ok, bool mark, int at, const MeshNoState&) {
            if (mark) {   // at < kept <= n_verts
                new_id[v] = at;
                const int e = move_edge[v];
                const float* p = e >= 0 ? edge_pos + 3 * (size_t)e : verts + 3 * v;
                verts_out[3 * (size_t)at + 0] = p[0];
                verts_out[3 * (size_t)at + 1] = p[1];
                verts_out[3 * (size_t)at + 2] = p[2];
                vert_src[at] = vsrc[v];
            }
            if (ok && v >= kept) {   // rows below `kept` are written by the vertices that land there, the others here
                verts_out[3 * v + 0] = 0.f;
                verts_out[3 * v + 1] = 0.f;
                verts_out[3 * v + 2] = 0.f;
                vert_src[v] = 0;
            }
        });
}

// the faces that stay, in order and orientation.  An id in [0, V) is renamed, another one stays as it is
struct MxFace {
    int id[3];
};

template <bool FILL>
__global__ __launch_bounds__(kImeshThreads) void k_mx_faces(const int* __restrict__ faces, int n_faces, int n_verts,
                                                            const int* __restrict__ merge_to, const int* __restrict__ new_id,
                                                            int* __restrict__ blk_count, const int* __restrict__ blk_base,
                                                            const int* __restrict__ counts, int* __restrict__ faces_out,
                                                            int* __restrict__ face_src) {
    const int kept = FILL ? counts[1] : 0;
    mesh_compact<FILL, MxFace>(
        n_faces, blk_count, blk_base,
        [&](long long f, MxFace& to) {
            bool named = true;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int id = faces[3 * f + c];
                const bool in = (unsigned)id < (unsigned)n_verts;
                named = named && in;
                to.id[c] = in ? merge_to[id] : id;
            }
            const int a = faces[3 * f + 0], b = faces[3 * f + 1], c = faces[3 * f + 2];
            const bool valid = named && a != b && b != c && a != c;
            return !(valid && (to.id[0] == to.id[1] || to.id[1] == to.id[2] || to.id[0] == to.id[2]));
        },
        [&](long long f, bool ok, bool mark, int at, const MxFace& to) {
            if (mark) {   // at < kept <= n_faces; a merged id lies in [0, V) exactly when the face's own id does
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const bool in = (unsigned)faces[3 * f + c] < (unsigned)n_verts;
                    faces_out[3 * (size_t)at + c] = in ? new_id[to.id[c]] : to.id[c];
                }
                face_src[at] = (int)f;
            }
            if (ok && f >= kept) {
                faces_out[3 * f + 0] = 0;
                faces_out[3 * f + 1] = 0;
                faces_out[3 * f + 2] = 0;
                face_src[f] = 0;
            }
        });
}

__global__ void k_mx_finish(int* __restrict__ counts, int need) {
    if (blockIdx.x == 0 && threadIdx.x == 0) counts[3] = min(counts[2], need);
}
