// meshsubdiv.hpp -- one round of subdivision of an indexed mesh, on the device: midpoint or Loop, every edge or the long ones.
//
// Reference: none (see meshsimp.hpp).  Everything else in the mesh toolkit keeps the vertex count or lowers it; this makes a mesh
// finer and keeps its connectivity story: old vertices keep their ids, the k-th marked edge in entry order becomes vertex V + k,
// a face with m marked edges becomes 1 + m faces in its own orientation.  The rule is meshing.mesh_subdivide_round: integers
// decide (marks, ranks, templates), positions are float64 from the float32 input with every operation rounded on its own, and
// Loop's weights are Warren's (no cosine), so the result is compared with the specification bit for bit.  Marks belong to edges:
// both faces on an edge see the same split and the result has no T-junction.
//
// arah_mesh_subdivide_round, one launch per line (after arah_mesh_adjacency's own, called on the input faces):
//
//   k_sb_owner          one thread per vertex: the owner of every neighbour entry
//   k_sb_face_entries   one thread per face: the entry of each of its three edges by binary search of `hi` in `lo`'s sorted neighbour
//                       segment (-1 for an invalid face); Loop: the third corner into slot 0 (the face traverses lo->hi) or 1 (hi->lo)
//                       of the edge's entry -- plain stores, one writer per slot of a regular edge, other slots are never read
//   k_sb_verts          one thread per old vertex: copied (midpoint) or classified and moved (Loop: interior, rim, kept) from the
//                       input positions; vert_src = (v, v); the per-workgroup numbers of interior and rim vertices
//   k_sb_marks<false>, k_mc_scan, k_sb_marks<true>
//                       count / scan / fill over the 6 F neighbour entries, one lane per entry: an edge (nbr > owner) is marked when
//                       the round is uniform or both ends are finite and d2 > max_len2; fill: rank (the new vertex is V + rank, -1
//                       without a mark), the new vertex's position and vert_src = (lo, hi)
//   k_sb_faces<false>, k_mc_scan, k_sb_faces<true>
//                       count / scan / fill over the faces with the weight 1 + m: the templates, face_src; the two-mark template's
//                       diagonal is decided on the OUTPUT positions, which the two passes above have written
//   k_sb_finish         the counts, from the scans' totals and the per-workgroup statistics
//   k_mc_pad_words      the rows past the counts zeroed
//
// NO ATOMICS of its own (the adjacency build's integer ones are the only ones): ranks come from mesh_prefix and k_mc_scan, the
// statistics from per-workgroup sums that one workgroup adds up.  No thread waits for another: no spin-wait, no grid-wide
// barrier; every loop ends by an argument of its own, stated at the loop.  MeshAdj is meshadj.hpp's; the owner fill, the entry's
// ends (ma_entry), the bisection (ma_find) and ma_finite / ma_d2 are meshedge.hpp's.
//
// NOT MEASURED AGAINST AN ALTERNATIVE: one lane per old vertex under Loop -- a fan's apex with n neighbours is summed by one
// lane, n additions in ascending id, where meshadj.hpp spreads a long segment over a workgroup; keeping the three entries of
// a face (12 bytes per face of scratch) instead of searching them again in each of the two face passes; the owner array
// (meshedge.hpp tells that one).
#pragma once

constexpr int kSbCounts = 13;   // meshing.SUBDIVIDE_COUNTS
constexpr int kSbLoop = 1;      // method: 0 midpoint, 1 Loop

__device__ __forceinline__ float sb_mid(float lo, float hi) {
#pragma clang fp contract(off)
    return (float)(((double)lo + (double)hi) * 0.5);
}

// Warren's edge rule: 3/8 of the ends, 1/8 of the two opposite corners
__device__ __forceinline__ float sb_loop_edge(float lo, float hi, float c, float d) {
#pragma clang fp contract(off)
    const double ends = ((double)lo + (double)hi) * 0.375;
    const double wings = ((double)c + (double)d) * 0.125;
    return (float)(ends + wings);
}

// an interior vertex: p (1 - k beta) + s beta
__device__ __forceinline__ float sb_loop_interior(float p, double s, double keep, double beta) {
#pragma clang fp contract(off)
    const double own = (double)p * keep;
    const double ring = s * beta;
    return (float)(own + ring);
}

// Warren's beta of a vertex with k neighbours, and what the vertex keeps of itself
__device__ __forceinline__ void sb_loop_weights(int k, double& beta, double& keep) {
#pragma clang fp contract(off)
    beta = k == 3 ? 0.1875 : 3.0 / (8.0 * (double)k);
    const double ring = (double)k * beta;
    keep = 1.0 - ring;
}

// a rim vertex: 3/4 of itself, 1/8 of its two rim neighbours
__device__ __forceinline__ float sb_loop_rim(float p, float b0, float b1) {
#pragma clang fp contract(off)
    const double own = (double)p * 0.75;
    const double ring = ((double)b0 + (double)b1) * 0.125;
    return (float)(own + ring);
}

// The count (FILL = false) or fill (FILL = true) walk of a workgroup over its chunk of the n elements, mesh_compact with a WEIGHT
// per element instead of a 0/1 mark and three statistics riding along:
//   weigh(i, state, stat) -> int   called for i < n only: the number of ids the element takes; may fill `state`, and `stat` with
//                                  three 10-bit fields of 0 or 1 (a pass sums 256 of them per field)
//   emit(i, ok, weight, id, state) FILL only, called by EVERY thread: ok = i < n, id = the first id of the element
// COUNT writes blk_count[block] = the weights of the chunk and blk_stat[3 block + 0 .. 2] = the sums of the fields.  Launch
// kImeshThreads threads and ceil(n / kImeshChunk) workgroups; n is workgroup-uniform, so every thread reaches mesh_prefix.
template <bool FILL, class State, class Weigh, class Emit>
__device__ __forceinline__ void sb_walk(long long n, int* __restrict__ blk_count, const int* __restrict__ blk_base,
                                        int* __restrict__ blk_stat, Weigh weigh, Emit emit) {
    __shared__ int wsum[kImeshThreads / 64];
    const long long first = (long long)blockIdx.x * kImeshChunk;
    int done = 0, s0 = 0, s1 = 0, s2 = 0;
#pragma unroll 1
    for (int z0 = 0; z0 < kImeshChunk; z0 += kImeshThreads) {   // terminates: kImeshChunk - z0 strictly decreases to 0
        const long long i = first + z0 + threadIdx.x;
        const bool ok = i < n;
        State state{};
        int stat = 0;
        const int weight = ok ? weigh(i, state, stat) : 0;
        int total;
        const int before = mesh_prefix(weight, wsum, total);
        if constexpr (FILL) {
            emit(i, ok, weight, blk_base[blockIdx.x] + done + before, state);
        } else {
            int st;
            mesh_prefix(stat, wsum, st);
            s0 += st & 1023;
            s1 += (st >> 10) & 1023;
            s2 += (st >> 20) & 1023;
        }
        done += total;
    }
    if (!FILL && threadIdx.x == 0) {
        blk_count[blockIdx.x] = done;
        blk_stat[3 * (size_t)blockIdx.x + 0] = s0;
        blk_stat[3 * (size_t)blockIdx.x + 1] = s1;
        blk_stat[3 * (size_t)blockIdx.x + 2] = s2;
    }
}

__global__ __launch_bounds__(kImeshThreads) void k_sb_owner(MeshAdj adj, int* __restrict__ owner) {
    const long long step = (long long)gridDim.x * blockDim.x;
    // terminates: n_verts - v strictly decreases (step >= 1) and the loop ends when it reaches 0
    for (long long v = (long long)blockIdx.x * blockDim.x + threadIdx.x; v < adj.n_verts; v += step) ma_fill_owner(adj, v, owner);
}

__global__ __launch_bounds__(kImeshThreads) void k_sb_face_entries(const int* __restrict__ faces, MeshAdj adj, int loop,
                                                                   int* __restrict__ fent, int* __restrict__ opp) {
    const long long step = (long long)gridDim.x * blockDim.x;
    // terminates: n_faces - f strictly decreases (step >= 1) and the loop ends when it reaches 0
    for (long long f = (long long)blockIdx.x * blockDim.x + threadIdx.x; f < adj.n_faces; f += step) {
        int id[3];
        const bool ok = ma_face_ok(faces, f, adj.n_verts, id);
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            int e = -1;
            if (ok) {
                const int s = id[j], d = id[(j + 1) % 3];
                e = ma_find(adj, min(s, d), max(s, d));
                if (loop && e >= 0) opp[2 * (size_t)e + (s < d ? 0 : 1)] = id[(j + 2) % 3];   // e < nbr_start[V] <= 6 F
            }
            fent[3 * f + j] = ok && e >= 0 ? e : -1;
        }
    }
}

// the old vertices.  The walk is sb_walk's COUNT pass with the weight 0: nothing is numbered, the positions are written on the
// way and the statistics (interior, rim) come out per workgroup
__global__ __launch_bounds__(kImeshThreads) void k_sb_verts(const float* __restrict__ verts, MeshAdj adj, int loop,
                             int* __restrict__ blk_count, int* __restrict__ blk_stat, float* __restrict__ verts_out,
                             int* __restrict__ vert_src) {
    sb_walk<false, MeshNoState>(
        adj.n_verts, blk_count, (const int*)nullptr, blk_stat,
        [&](long long v, MeshNoState&, int& stat) {
            const float p[3] = {verts[3 * v + 0], verts[3 * v + 1], verts[3 * v + 2]};
            float out[3] = {p[0], p[1], p[2]};
            if (loop && ma_finite(verts, v)) {
                const int first = adj.nbr_start[v], last = adj.nbr_start[v + 1], k = last - first;
                bool all_regular = true, others_regular = true, all_finite = true;
                int n_one = 0, rim[2] = {-1, -1};
                double s[3] = {0.0, 0.0, 0.0};
                for (int i = first; i < last; ++i) {   // terminates: last - i strictly decreases
                    const int n = adj.nbr[i], n_out = adj.nbr_out[i], n_in = adj.nbr_in[i];
                    const bool regular = n_out == 1 && n_in == 1, one = n_out + n_in == 1;
                    all_regular = all_regular && regular;
                    others_regular = others_regular && (regular || one);
                    if (one) {
                        if (n_one < 2) rim[n_one] = n;
                        ++n_one;
                    }
                    all_finite = all_finite && ma_finite(verts, n);   // n is a vertex of a valid face: in [0, V)
                    s[0] = s[0] + (double)verts[3 * (size_t)n + 0];
                    s[1] = s[1] + (double)verts[3 * (size_t)n + 1];
                    s[2] = s[2] + (double)verts[3 * (size_t)n + 2];
                }
                if (k > 0 && all_regular && all_finite) {
                    double beta, keep;
                    sb_loop_weights(k, beta, keep);
#pragma unroll
                    for (int a = 0; a < 3; ++a) out[a] = sb_loop_interior(p[a], s[a], keep, beta);
                    stat = 1;
                } else if (n_one == 2 && others_regular && ma_finite(verts, rim[0]) && ma_finite(verts, rim[1])) {
#pragma unroll
                    for (int a = 0; a < 3; ++a)
                        out[a] = sb_loop_rim(p[a], verts[3 * (size_t)rim[0] + a], verts[3 * (size_t)rim[1] + a]);
                    stat = 1 << 10;
                }
            }
            verts_out[3 * v + 0] = out[0];
            verts_out[3 * v + 1] = out[1];
            verts_out[3 * v + 2] = out[2];
            vert_src[2 * v + 0] = (int)v;
            vert_src[2 * v + 1] = (int)v;
            return 0;
        },
        [](long long, bool, int, int, const MeshNoState&) {});
}

struct SbMark {
    bool finite;
};

// the marked edges in entry order; FILL: their ranks, positions and sources
template <bool FILL>
__global__ __launch_bounds__(kImeshThreads) void k_sb_marks(const float* __restrict__ verts, MeshAdj adj, int n_entries_cap,
                                                            const int* __restrict__ owner, const int* __restrict__ opp, int loop,
                                                            int has_threshold, double max_len2, int* __restrict__ blk_count,
                                                            const int* __restrict__ blk_base, int* __restrict__ blk_stat,
                                                            int* __restrict__ rank, float* __restrict__ verts_out,
                                                            int* __restrict__ vert_src) {
    const int n_verts = adj.n_verts, n_entries = adj.nbr_start[n_verts];
    sb_walk<FILL, SbMark>(
        n_entries_cap, blk_count, blk_base, blk_stat,
        [&](long long i, SbMark& st, int& stat) {
            int u, v;
            if (i >= n_entries || !ma_entry(adj, owner, i, u, v)) return 0;
            st.finite = ma_finite(verts, u) && ma_finite(verts, v);
            const bool marked = has_threshold ? st.finite && ma_d2(verts + 3 * (size_t)u, verts + 3 * (size_t)v) > max_len2 : true;
            stat = marked && !st.finite ? 1 : 0;
            return marked ? 1 : 0;
        },
        [&](long long i, bool ok, int weight, int at, const SbMark& st) {
            if (!ok) return;
            rank[i] = weight ? at : -1;
            if (!weight) return;
            // at < the marked edges <= the edges <= 3 F: the row lies below V + 3 F
            const int u = owner[i], v = adj.nbr[i];
            const size_t row = (size_t)n_verts + (size_t)at;
            const float *lo = verts + 3 * (size_t)u, *hi = verts + 3 * (size_t)v;
            float out[3];
            if (!st.finite) {   // a copy of the lowest non-finite end: no arithmetic touches a NaN's payload
                const float* src = ma_finite(verts, u) ? hi : lo;
                out[0] = src[0], out[1] = src[1], out[2] = src[2];
            } else {
                bool stencil = false;
                int c = 0, d = 0;
                if (loop && adj.nbr_out[i] == 1 && adj.nbr_in[i] == 1) {   // a regular edge: each slot was written by its one face
                    c = opp[2 * (size_t)i + 0], d = opp[2 * (size_t)i + 1];
                    stencil = (unsigned)c < (unsigned)n_verts && (unsigned)d < (unsigned)n_verts && ma_finite(verts, c) && ma_finite(verts,
                               d);
                }
#pragma unroll
                for (int a = 0; a < 3; ++a)
                    out[a] = stencil ? sb_loop_edge(lo[a], hi[a], verts[3 * (size_t)c + a], verts[3 * (size_t)d + a]) : sb_mid(lo[a], hi[a]);
            }
            verts_out[3 * row + 0] = out[0];
            verts_out[3 * row + 1] = out[1];
            verts_out[3 * row + 2] = out[2];
            vert_src[2 * row + 0] = u;
            vert_src[2 * row + 1] = v;
        });
}

struct SbFace {
    int nv[3];   // the new vertices on ab, bc, ca, or -1
    int m;       // marked edges; -1: an invalid face
};

__device__ __forceinline__ void sb_put_face(int* __restrict__ faces_out, int* __restrict__ face_src, size_t row, int a, int b, int c,
                                            long long f) {
    faces_out[3 * row + 0] = a;
    faces_out[3 * row + 1] = b;
    faces_out[3 * row + 2] = c;
    face_src[row] = (int)f;
}

// the faces by their templates, in the order of the input faces
template <bool FILL>
__global__ __launch_bounds__(kImeshThreads) void k_sb_faces(const int* __restrict__ faces, int n_faces, int n_verts,
                                                            const int* __restrict__ fent, const int* __restrict__ rank,
                                                            int* __restrict__ blk_count, const int* __restrict__ blk_base,
                                                            int* __restrict__ blk_stat, const float* __restrict__ pos,
                                                            int* __restrict__ faces_out, int* __restrict__ face_src) {
    sb_walk<FILL, SbFace>(
        n_faces, blk_count, blk_base, blk_stat,
        [&](long long f, SbFace& st, int& stat) {
            if (fent[3 * f] < 0) {
                st.m = -1;
                return 1;
            }
            st.m = 0;
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const int e = fent[3 * f + j];
                const int r = e >= 0 ? rank[e] : -1;
                st.nv[j] = r >= 0 ? n_verts + r : -1;   // V + r < V + 3 F < 2^31
                st.m += r >= 0 ? 1 : 0;
            }
            stat = st.m == 1 ? 1 : st.m == 2 ? 1 << 10 : st.m == 3 ? 1 << 20 : 0;
            return 1 + st.m;
        },
        [&](long long f, bool ok, int weight, int at, const SbFace& st) {
            if (!ok) return;
            // rows at .. at + weight - 1 lie below the faces out <= 4 F
            const size_t row = (size_t)at;
            const int id[3] = {faces[3 * f + 0], faces[3 * f + 1], faces[3 * f + 2]};
            if (st.m <= 0) {
                sb_put_face(faces_out, face_src, row, id[0], id[1], id[2], f);
                return;
            }
            if (st.m == 3) {
                const int a = id[0], b = id[1], c = id[2], x = st.nv[0], y = st.nv[1], z = st.nv[2];
                sb_put_face(faces_out, face_src, row + 0, a, x, z, f);
                sb_put_face(faces_out, face_src, row + 1, x, b, y, f);
                sb_put_face(faces_out, face_src, row + 2, z, y, c, f);
                sb_put_face(faces_out, face_src, row + 3, x, y, z, f);
                return;
            }
            // one mark: rotate so that ab carries it; two marks: so that ca carries none
            int r = 0;
            if (st.m == 1) r = st.nv[0] >= 0 ? 0 : st.nv[1] >= 0 ? 1 : 2;
            else r = st.nv[2] < 0 ? 0 : st.nv[0] < 0 ? 1 : 2;
            const int a = id[r], b = id[(r + 1) % 3], c = id[(r + 2) % 3], x = st.nv[r], y = st.nv[(r + 1) % 3];
            if (st.m == 1) {
                sb_put_face(faces_out, face_src, row + 0, a, x, c, f);
                sb_put_face(faces_out, face_src, row + 1, x, b, c, f);
                return;
            }
            sb_put_face(faces_out, face_src, row + 0, x, b, y, f);
            // the quad a, x, y, c along its shorter diagonal, ties to x-c; all four are vertices of the output
            const bool ay = ma_d2(pos + 3 * (size_t)a, pos + 3 * (size_t)y) < ma_d2(pos + 3 * (size_t)x, pos + 3 * (size_t)c);
            if (ay) {
                sb_put_face(faces_out, face_src, row + 1, a, x, y, f);
                sb_put_face(faces_out, face_src, row + 2, a, y, c, f);
            } else {
                sb_put_face(faces_out, face_src, row + 1, a, x, c, f);
                sb_put_face(faces_out, face_src, row + 2, x, y, c, f);
            }
        });
}

// counts, by one workgroup: the totals of the two scans (null: the walk did not run) and the sums of the per-workgroup
// statistics of the three walks (integer sums: the order does not show)
__global__ __launch_bounds__(kImeshThreads) void k_sb_finish(int n_verts, int n_faces, const int* __restrict__ acounts,
                                                             const int* __restrict__ n_marked, const int* __restrict__ n_faces_out,
                                                             const int* __restrict__ vert_stat, int vert_blocks,
                                                             const int* __restrict__ mark_stat, int mark_blocks,
                                                             const int* __restrict__ face_stat, int face_blocks, int* __restrict__ counts) {
    __shared__ int red[6][kImeshThreads];
    int sum[6] = {0, 0, 0, 0, 0, 0};   // interior, rim, marked with a non-finite end, faces with 1, 2, 3 marks
    for (int b = threadIdx.x; b < vert_blocks; b += kImeshThreads) {   // terminates: vert_blocks - b strictly decreases
        sum[0] += vert_stat[3 * (size_t)b + 0];
        sum[1] += vert_stat[3 * (size_t)b + 1];
    }
    for (int b = threadIdx.x; b < mark_blocks; b += kImeshThreads) sum[2] += mark_stat[3 * (size_t)b + 0];   // terminates: as above
    for (int b = threadIdx.x; b < face_blocks; b += kImeshThreads) {   // terminates: as above
        sum[3] += face_stat[3 * (size_t)b + 0];
        sum[4] += face_stat[3 * (size_t)b + 1];
        sum[5] += face_stat[3 * (size_t)b + 2];
    }
    for (int j = 0; j < 6; ++j) red[j][threadIdx.x] = sum[j];
    __syncthreads();
    for (int s = kImeshThreads / 2; s > 0; s >>= 1) {   // terminates: s halves down to 0
        if ((int)threadIdx.x < s)
            for (int j = 0; j < 6; ++j) red[j][threadIdx.x] += red[j][threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const int marked = n_marked ? *n_marked : 0, valid = acounts[0];
        const int f1 = red[3][0], f2 = red[4][0], f3 = red[5][0];
        counts[0] = n_verts + marked;
        counts[1] = n_faces_out ? *n_faces_out : 0;
        counts[2] = acounts[1];
        counts[3] = marked;
        counts[4] = valid - f1 - f2 - f3;
        counts[5] = f1;
        counts[6] = f2;
        counts[7] = f3;
        counts[8] = n_faces - valid;
        counts[9] = red[2][0];
        counts[10] = red[0][0];
        counts[11] = red[1][0];
        counts[12] = n_verts - red[0][0] - red[1][0];
    }
}
