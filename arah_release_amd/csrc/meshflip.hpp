// meshflip.hpp -- one round of edge flips of an indexed mesh, on the device.
//
// Reference: none (see meshsimp.hpp).  A flip replaces the edge {u, v} between the faces (u, v, a) and (v, u, b) by the edge
// {a, b} between (a, u, b) and (b, v, a): the vertices, the face count and the surface's topology stay, the connectivity changes.
// It is the step that improves triangles without moving anything: towards the Delaunay triangulation of the surface (the edge
// goes when the two angles opposite to it sum to more than pi), or towards valence six (Botsch and Kobbelt's remeshing).  The
// rule is meshing.mesh_flip_round, float64 with every operation rounded on its own and no square root; every decision is taken
// on integers or on the comparison of two rounded numbers, so the result is compared with it bit for bit.
//
// THE DELAUNAY TEST IS ASKED BOTH WAYS.  cot + cot < 0 is decided as a comparison of products of rounded numbers.  The four
// angles of a quad in space sum to at most 2 pi, so exactly, an edge and its flip never both fail; rounded, a nearly
// co-circular quad can fail both ways, and a marching-cubes mesh is full of such quads: on the 33^3 sphere 21 edges flipped
// back and forth for ever.  So an edge flips only when it asks to go and its flip would not ask to come back.  The valence
// criterion needs nothing of the kind: every flip strictly lowers an integer that is bounded below.
//
// MANY FLIPS PER ROUND, INDEPENDENT OF THE ORDER OF ARRIVAL.  key(e) = (hash32(id ^ salt 0x9e3779b9) << 32) | id is unique, for
// the id is.  Every candidate takes atomicMin(key) into lock[x] of its four vertices Q(e) = {u, v, a, b}; it is selected when
// all four locks hold its key.  Two selected flips e, e' with a common vertex x have key(e) = lock[x] = key(e'), so e = e':
// SELECTED FLIPS HAVE DISJOINT QUADRUPLES.  It follows that
//   * they rewrite disjoint faces: the two faces of e have their corners in Q(e), those of e' in Q(e');
//   * no two create the same edge: {a, b} lies in Q(e), {a', b'} in Q(e');
//   * every test e passed still holds when it is applied together with the others.  The faces that name both u and v (one each
//     way, their third corners a and b) are faces with two corners in Q(e): a face e' rewrites has all three in Q(e'), before and
//     after.  "{a, b} is no edge" could only fail by a new edge with both ends in Q(e).  The valences and boundary flags of Q(e)
//     change only by flips that have one of these vertices in their own quadruple.  Positions never change.
// Minima over integers do not depend on the order of arrival.  The hash is there for the number of rounds, not for correctness:
// ids of a marching-cubes mesh are spatially coherent, so with the bare id as the key nearly every candidate is blocked by a
// neighbour with a lower id; the salt (the round number) changes the order from round to round.
//
// arah_mesh_flip_round, one launch per line (after arah_mesh_adjacency's own, called on the current faces):
//
//   k_mf_init      one thread per vertex: the owner of every neighbour entry, lock = empty; one thread per face: the row copied,
//                  its flag cleared; counts cleared
//   k_mf_edge      one LANE per neighbour entry with nbr > owner: the two faces and third corners by a merge of the two face
//                  segments, a binary search of b in a's sorted neighbours, the criterion, the four dot products; writes key and
//                  reason; atomicMin of the key into the locks of u, v, a, b; the reasons counted
//   k_mf_apply     one lane per entry that holds a key: selected when the four locks hold it (the third corners by the merge
//                  once more); the two rows rewritten and flagged -- one writer per row, see above; the selected counted
//
// Integer atomics only (min, add).  No thread waits for another: no spin-wait, no grid-wide barrier; every loop ends by an
// argument of its own, stated at the loop.  MeshAdj is meshadj.hpp's; the owner fill, the entry walk, the bisection (ma_find),
// the merge (MaMerge) and the float64 helpers (ma_load, ma_dot, ma_cross) are meshedge.hpp's.
//
// NOT MEASURED AGAINST AN ALTERNATIVE (nothing here has been timed against another way of doing it): one lane per entry (half
// the entries name no edge and their lanes idle; the lanes of a wave diverge on the reason and on the segment lengths -- a
// compacted list of the edges, or a wave per edge, are the alternatives); the four-vertex lock against meshcollapse.hpp's
// two-pass minimum over closed neighbourhoods (which selects fewer flips per round but needs no third corners in the second
// pass); finding the third corners again in k_mf_apply instead of keeping four ids per entry in scratch; the owner array
// (meshedge.hpp tells that one).
#pragma once

constexpr unsigned long long kMfEmpty = ~0ull;   // no key: an id is below 2^31, so no key is all ones
constexpr int kMfNoEdge = 255;                   // edge_reason of an entry that names no edge
constexpr int kMfCounts = 9;                     // edges, candidates, selected, six reasons
constexpr int kMfValence = 1;                    // criterion: 0 delaunay, 1 valence

// a two-round multiply-xorshift finaliser of 32-bit integers (a bijection); meshing.flip_hash32
__device__ __forceinline__ unsigned mf_hash32(unsigned x) {
    x ^= x >> 16;
    x *= 0x7feb352du;
    x ^= x >> 15;
    x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}

// The faces that name both u and v, by the merge of the two ascending face segments: fa traverses u->v and has the third corner
// a, fb traverses v->u and has the third corner b.  -> the number of such faces; the four ids are the first of each kind (-1
// without one).  The callers have nbr_out = nbr_in = 1 for the entry, so there is exactly one of each kind.
__device__ __forceinline__ int mf_wings(const int* __restrict__ faces, const MeshAdj& adj, int u, int v, int& fa, int& a, int& fb,
                                        int& b) {
    fa = a = fb = b = -1;
    int shared = 0;
    bool both;
    MaMerge w = ma_merge(adj.vf, adj.vf_start, u, v);
    while (ma_more(w)) {   // terminates: every call consumes an element of the two segments
        const int f = ma_next(w, both);
        if (!both) continue;   // a valid face of this mesh: its ids lie in [0, V) and two of them are u and v
        const int i0 = faces[3 * (size_t)f + 0], i1 = faces[3 * (size_t)f + 1], i2 = faces[3 * (size_t)f + 2];
        const bool fwd = (i0 == u && i1 == v) || (i1 == u && i2 == v) || (i2 == u && i0 == v);
        const int third = i0 + i1 + i2 - u - v;
        if (fwd && fa < 0) {
            fa = f;
            a = third;
        } else if (!fwd && fb < 0) {
            fb = f;
            b = third;
        }
        ++shared;
    }
    return shared;
}

// The Delaunay test of the edge {s, t} with the opposite corners x and y, whose faces have the cross products Nx and Ny (any
// sign): d = (s - c) . (t - c) and c = |N|^2 at each corner c; true when the two opposite angles sum to more than pi --
// both d negative, or (d_n d_n) c_o > (d_o d_o) c_n with n the corner whose d is negative and o the other.  Not a number: false
__device__ __forceinline__ bool mf_wants(const double s[3], const double t[3], const double x[3], const double y[3], const double Nx[3],
                                         const double Ny[3]) {
#pragma clang fp contract(off)
    double sx[3], tx[3], sy[3], ty[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        sx[c] = s[c] - x[c];
        tx[c] = t[c] - x[c];
        sy[c] = s[c] - y[c];
        ty[c] = t[c] - y[c];
    }
    const double dx = ma_dot(sx, tx), dy = ma_dot(sy, ty);
    const double cx = ma_dot(Nx, Nx), cy = ma_dot(Ny, Ny);
    const double lhs = (dx * dx) * cy, rhs = (dy * dy) * cx;
    if (dx < 0.0 && dy < 0.0) return true;
    if (dx < 0.0 && dy >= 0.0) return lhs > rhs;
    if (dy < 0.0 && dx >= 0.0) return rhs > lhs;
    return false;
}

__global__ __launch_bounds__(kImeshThreads) void k_mf_init(const int* __restrict__ faces, MeshAdj adj, int* __restrict__ owner,
                                                           unsigned long long* __restrict__ lock, int* __restrict__ faces_out,
                                                           unsigned char* __restrict__ face_flag, int* __restrict__ counts) {
    if (blockIdx.x == 0 && threadIdx.x < kMfCounts) counts[threadIdx.x] = 0;
    const long long step = (long long)gridDim.x * blockDim.x;
    // terminates: n_verts - v strictly decreases (step >= 1) and the loop ends when it reaches 0
    for (long long v = (long long)blockIdx.x * blockDim.x + threadIdx.x; v < adj.n_verts; v += step) {
        ma_fill_owner(adj, v, owner);
        lock[v] = kMfEmpty;
    }
    // terminates: n_faces - f strictly decreases (step >= 1) and the loop ends when it reaches 0
    for (long long f = (long long)blockIdx.x * blockDim.x + threadIdx.x; f < adj.n_faces; f += step) {
        faces_out[3 * f + 0] = faces[3 * f + 0];
        faces_out[3 * f + 1] = faces[3 * f + 1];
        faces_out[3 * f + 2] = faces[3 * f + 2];
        face_flag[f] = 0;
    }
}

__global__ __launch_bounds__(kImeshThreads) void k_mf_edge(const float* __restrict__ verts, const int* __restrict__ faces, MeshAdj adj,
                                                           int n_entries_cap, const int* __restrict__ owner, int criterion, unsigned salt_mix,
                                                           unsigned long long* __restrict__ edge_key, unsigned char* __restrict__ edge_reason,
                                                           unsigned long long* lock, int* counts) {
#pragma clang fp contract(off)
    ma_entry_walk(adj, owner, n_entries_cap, [&](long long i, bool is_edge, int u, int v) {
#pragma clang fp contract(off)
        int reason = 0;
        unsigned long long key = kMfEmpty;
        if (is_edge) {
            int fa, a, fb, b;
            if (adj.nbr_out[i] != 1 || adj.nbr_in[i] != 1) {
                reason = 1;
            } else if (mf_wings(faces, adj, u, v, fa, a, fb, b) != 2 || fa < 0 || fb < 0 || a == b) {
                reason = 2;   // one face each way: two shared faces, one of each kind -- only a = b can hold here
            } else {
                const bool is_edge_ab = ma_find(adj, a, b) >= 0;
                double pu[3], pv[3], pa[3], pb[3];
                bool finite = true;
                ma_load(verts, u, pu, finite);
                ma_load(verts, v, pv, finite);
                ma_load(verts, a, pa, finite);
                ma_load(verts, b, pb, finite);
                if (is_edge_ab) {
                    reason = 3;
                } else if (!finite) {
                    reason = 4;
                } else {
                    double Na[3], Nb[3], N1[3], N2[3];
                    ma_cross(pa, pu, pv, Na);
                    ma_cross(pb, pv, pu, Nb);
                    ma_cross(pa, pu, pb, N1);
                    ma_cross(pb, pv, pa, N2);
                    bool asks;
                    if (criterion == kMfValence) {
                        const int q[4] = {u, v, a, b};
                        int before = 0, after = 0;
#pragma unroll
                        for (int k = 0; k < 4; ++k) {
                            const int off = (adj.nbr_start[q[k] + 1] - adj.nbr_start[q[k]]) - ((adj.vert_flags[q[k]] & 1) ? 4 : 6);
                            before += abs(off);
                            after += abs(off + (k < 2 ? -1 : 1));
                        }
                        asks = after < before;
                    } else {
                        // the edge asks to go, and the flipped edge {a, b} with the corners u, v does not ask to come back
                        asks = mf_wants(pu, pv, pa, pb, Na, Nb) && !mf_wants(pa, pb, pu, pv, N1, N2);
                    }
                    if (!asks) {
                        reason = 5;
                    } else {
                        const bool good = ma_dot(N1, Na) > 0.0 && ma_dot(N1, Nb) > 0.0 && ma_dot(N2, Na) > 0.0 && ma_dot(N2, Nb) > 0.0;
                        if (!good) {
                            reason = 6;
                        } else {   // u, v, a, b are ids of valid faces: all in [0, V)
                            key = ((unsigned long long)mf_hash32((unsigned)i ^ salt_mix) << 32) | (unsigned long long)i;
                            atomicMin(&lock[u], key);
                            atomicMin(&lock[v], key);
                            atomicMin(&lock[a], key);
                            atomicMin(&lock[b], key);
                        }
                    }
                }
            }
        }
        if (i < n_entries_cap) {
            edge_key[i] = key;
            edge_reason[i] = (unsigned char)(is_edge ? reason : kMfNoEdge);
        }
        cc_add_one(counts, 0, is_edge);
        cc_add_one(counts, reason == 0 ? 1 : 2 + reason, is_edge);   // candidates at 1, reason r <= 6 at 2 + r <= 8
    });
}

__global__ __launch_bounds__(kImeshThreads) void k_mf_apply(const int* __restrict__ faces, MeshAdj adj, int n_entries_cap,
                                                            const int* __restrict__ owner, const unsigned long long* __restrict__ edge_key,
                                                            const unsigned long long* __restrict__ lock, int* __restrict__ faces_out,
                                                            unsigned char* __restrict__ face_flag, int* counts) {
    ma_walk(adj, n_entries_cap, [&](long long i, bool live) {
        bool selected = false;
        const unsigned long long key = live ? edge_key[i] : kMfEmpty;
        if (key != kMfEmpty) {   // a candidate: an edge with one face each way and two different third corners
            const int u = owner[i], v = adj.nbr[i];
            if (lock[u] == key && lock[v] == key) {
                int fa, a, fb, b;
                mf_wings(faces, adj, u, v, fa, a, fb, b);
                if (lock[a] == key && lock[b] == key) {   // selected flips share no vertex: every row has one writer
                    selected = true;
                    faces_out[3 * (size_t)fa + 0] = a;
                    faces_out[3 * (size_t)fa + 1] = u;
                    faces_out[3 * (size_t)fa + 2] = b;
                    faces_out[3 * (size_t)fb + 0] = b;
                    faces_out[3 * (size_t)fb + 1] = v;
                    faces_out[3 * (size_t)fb + 2] = a;
                    face_flag[fa] = 1;
                    face_flag[fb] = 1;
                }
            }
        }
        cc_add_one(counts, 2, selected);
    });
}
