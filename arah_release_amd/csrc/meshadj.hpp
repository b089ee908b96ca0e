// meshadj.hpp -- adjacency of an indexed mesh on the device, and the gathers that run over it: per-vertex normals, umbrella
// (Laplacian / Taubin) smoothing, and the tangential step of the isotropic remesher (k_ma_tangential, arah_mesh_tangential).
//
// Reference: none in its tree.  The reference's users smooth and re-normal their meshes with trimesh / open3d / pytorch3d
// (Meshes.verts_normals_packed: the area-weighted sum of the incident faces' cross products, the definition taken here); none of
// them is a dependency of this project.  All three need to know who is adjacent to whom, and every result is defined so that
// it is unique and compared bit for bit with the tensor specification (meshing.mesh_adjacency / vertex_normals / mesh_smooth):
//
//   * a face is VALID when its three ids lie in [0, V) and are pairwise different; a valid face (a, b, c) traverses a->b, b->c,
//     c->a;
//   * vf: the valid faces incident to every vertex as a CSR, face ids ASCENDING within a vertex;
//   * nbr: the UNIQUE neighbours of every vertex as a CSR, ids ascending, with the number of faces traversing v->n (nbr_out) and
//     n->v (nbr_in); an undirected edge is seen once, from its lower end (n > v), with nbr_out + nbr_in faces on it;
//   * normals: float64 cross products summed per vertex in ascending face id, contraction off -- a gather, no atomics;
//   * smoothing: float64 sums of the finite neighbours in ascending id, contraction off, two buffers -- a gather, no atomics;
//   * the tangential step: the same sums, then the move minus its part along the vertex's normal_sum, by one division and no square
//     root (meshing.mesh_tangential_step) -- a gather, no atomics.
//
// arah_mesh_adjacency, one launch per line:
//
//   k_ma_init        deg, cursor (one int per vertex each) and counts cleared
//   k_ma_count       one thread per face: deg[id] += 1 for the three ids of a valid face; counts[0] = the valid faces
//   k_mc_scan        vf_start = the exclusive scan of deg, vf_start[V] = the total
//   k_ma_fill        one thread per face: slot = vf_start[id] + cursor[id]++ for each corner; the face id goes to vf_raw[slot], the
//                    corner's two directed edges as (other id << 1) | (0: leaves the corner, 1: arrives) to nb_raw[2 slot + 0 / 1].
//                    The ORDER inside a vertex's segment is the order of arrival -- and the next two lines sort it away
//   k_ma_sort_short  one thread per vertex, segments of at most kMaShort elements: rank-count sort vf_raw -> vf and nb_raw -> nb_sorted
//   k_ma_sort_long   one workgroup per longer segment (a fan's apex, a badly clustered mesh), the same rank-count sort with the
//                    elements spread over the threads: n^2 / 256 comparisons per thread instead of n^2 in one lane
//   k_ma_nbr<false>  one thread per vertex: walks its sorted edges, counts the runs of equal neighbour ids -> deg (reused)
//   k_mc_scan        nbr_start, nbr_start[V]
//   k_ma_nbr<true>   the same walk: nbr, nbr_out, nbr_in, vert_flags; the edge statistics from the entries with n > v
//   k_mc_pad_words   the rows of vf from vf_start[V] on and of nbr / nbr_out / nbr_in from nbr_start[V] on zeroed
//   k_ma_finish      counts[7], the Euler characteristic
//
// Integer atomics only (add, max).  Their order of arrival decides the layout of vf_raw and nb_raw and nothing else, and both
// are sorted before anything reads them, ties between equal edge keys broken by position -- equal keys are interchangeable.  No
// thread waits for another: no spin-wait, no grid-wide barrier; every loop ends by an argument of its own, stated at the loop.
// kImeshThreads, kImeshMaxGrid, k_mc_scan and k_mc_pad_words are meshcommon.hpp's.
//
// WHAT THE OTHER HEADERS TAKE FROM HERE: MeshAdj, the device view of the eight arrays, which the kernels of a round (collapse,
// flip, subdivide) take by value, and ma_face_ok.  The build kernels below keep their own arguments: they write the arrays.  The
// three gathers at the end of this file and the kernels of meshlaplace.hpp keep theirs too: each runs for 5 to 8 us on 50 k
// vertices and took 0.5 us longer with the view's larger argument block, its instructions after the argument loads unchanged
// (profiles/mesh_adj_bench.txt).  What is done WITH the view -- the owner of an entry, the walk over the entries, the bisection
// of a neighbour segment, the merge of two segments, the float64 helpers -- is meshedge.hpp's, included right after this file.
#pragma once

constexpr int kMaShort = 32;              // elements of a segment one thread still sorts alone: at most 32^2 comparisons
constexpr int kMaLongGrid = 1024;         // workgroups that share the long segments

// The adjacency as the kernels of a round see it: the eight arrays of arah_mesh_adjacency and the sizes they were built for.  The
// round's entry carves the arrays from its own scratch and builds them (the host side: carve_mesh_adj, mesh_adj_build), so they
// are trusted: segments are not clamped and ids are followed.
struct MeshAdj {
    const int *vf_start, *vf, *nbr_start, *nbr, *nbr_out, *nbr_in;
    const unsigned char* vert_flags;
    const int* counts;
    int n_verts, n_faces;
};

// the three ids of face f when it is valid: in range and pairwise different
__device__ __forceinline__ bool ma_face_ok(const int* __restrict__ faces, long long f, int n_verts, int id[3]) {
    return cc_face_ok(faces, f, n_verts, id) && id[0] != id[1] && id[1] != id[2] && id[0] != id[2];
}

__global__ __launch_bounds__(kImeshThreads) void k_ma_init(int* __restrict__ deg, int* __restrict__ cursor, int n_verts,
                                                           int* __restrict__ counts) {
    const long long step = (long long)gridDim.x * blockDim.x;
    // terminates: n_verts - v strictly decreases (step >= 1) and the loop ends when it reaches 0
    for (long long v = (long long)blockIdx.x * blockDim.x + threadIdx.x; v < n_verts; v += step) {
        deg[v] = 0;
        cursor[v] = 0;
    }
    if (blockIdx.x == 0 && threadIdx.x < 8) counts[threadIdx.x] = 0;
}

__global__ __launch_bounds__(kImeshThreads) void k_ma_count(const int* __restrict__ faces, int n_faces, int n_verts, int* deg, int* counts) {
    const long long step = (long long)gridDim.x * blockDim.x, end = ((long long)n_faces + 63) & ~63ll;
    // terminates: end - f strictly decreases (step >= 1) and the loop ends when it reaches 0.  The face count is rounded up to
    // whole waves so that every lane reaches the ballot; lanes beyond the end carry no face
    for (long long f = (long long)blockIdx.x * blockDim.x + threadIdx.x; f < end; f += step) {
        int id[3];
        const bool ok = f < n_faces && ma_face_ok(faces, f, n_verts, id);
        if (ok) {
            atomicAdd(&deg[id[0]], 1);
            atomicAdd(&deg[id[1]], 1);
            atomicAdd(&deg[id[2]], 1);
        }
        const unsigned long long n_ok = __ballot(ok);
        if ((threadIdx.x & 63) == 0 && n_ok) atomicAdd(&counts[0], (int)__popcll(n_ok));
    }
}

__global__ __launch_bounds__(kImeshThreads) void k_ma_fill(const int* __restrict__ faces, int n_faces, int n_verts,
                                                           const int* __restrict__ vf_start, int* cursor, unsigned* __restrict__ vf_raw,
                                                           unsigned* __restrict__ nb_raw) {
    const long long step = (long long)gridDim.x * blockDim.x;
    // terminates: n_faces - f strictly decreases (step >= 1) and the loop ends when it reaches 0
    for (long long f = (long long)blockIdx.x * blockDim.x + threadIdx.x; f < n_faces; f += step) {
        int id[3];
        if (!ma_face_ok(faces, f, n_verts, id)) continue;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            // a vertex takes exactly deg[v] = vf_start[v + 1] - vf_start[v] slots, one per corner k_ma_count counted: slot < 3 F
            const long long slot = (long long)vf_start[id[c]] + atomicAdd(&cursor[id[c]], 1);
            vf_raw[slot] = (unsigned)f;
            nb_raw[2 * slot + 0] = ((unsigned)id[(c + 1) % 3] << 1) | 0u;   // corner -> next
            nb_raw[2 * slot + 1] = ((unsigned)id[(c + 2) % 3] << 1) | 1u;   // previous -> corner
        }
    }
}

// Rank-count sort of src[0 .. n) into dst[0 .. n): element i goes to the number of elements in front of it, equal ones by
// position.  The ranks are a permutation of 0 .. n - 1, so every dst row is written exactly once and src is only read.  The
// calling threads share the elements: thread `tid` of `nthreads` takes i = tid, tid + nthreads, ...
__device__ __forceinline__ void ma_rank_sort(const unsigned* __restrict__ src, unsigned* __restrict__ dst, int n, int tid, int nthreads) {
    // terminates: n - i strictly decreases (nthreads >= 1); the inner loop runs n times
    for (int i = tid; i < n; i += nthreads) {
        const unsigned x = src[i];
        int rank = 0;
        for (int j = 0; j < n; ++j) {
            const unsigned y = src[j];
            rank += (y < x || (y == x && j < i)) ? 1 : 0;
        }
        dst[rank] = x;
    }
}

__global__ __launch_bounds__(kImeshThreads) void k_ma_sort_short(const int* __restrict__ vf_start, int n_verts,
                                                                 const unsigned* __restrict__ vf_raw, unsigned* __restrict__ vf,
                                                                 const unsigned* __restrict__ nb_raw, unsigned* __restrict__ nb_sorted) {
    const long long step = (long long)gridDim.x * blockDim.x;
    // terminates: n_verts - v strictly decreases (step >= 1) and the loop ends when it reaches 0
    for (long long v = (long long)blockIdx.x * blockDim.x + threadIdx.x; v < n_verts; v += step) {
        const long long s = vf_start[v];
        const int n = (int)(vf_start[v + 1] - s);
        if (n <= kMaShort) ma_rank_sort(vf_raw + s, vf + s, n, 0, 1);
        if (2 * n <= kMaShort) ma_rank_sort(nb_raw + 2 * s, nb_sorted + 2 * s, 2 * n, 0, 1);
    }
}

__global__ __launch_bounds__(kImeshThreads) void k_ma_sort_long(const int* __restrict__ vf_start, int n_verts,
                                                                const unsigned* __restrict__ vf_raw, unsigned* __restrict__ vf,
                                                                const unsigned* __restrict__ nb_raw, unsigned* __restrict__ nb_sorted) {
    // terminates: n_verts - v strictly decreases (gridDim.x >= 1) and the loop ends when it reaches 0.  v and n are the same
    // for every thread of the workgroup; nothing is shared between its threads but the read-only source
    for (long long v = blockIdx.x; v < n_verts; v += gridDim.x) {
        const long long s = vf_start[v];
        const int n = (int)(vf_start[v + 1] - s);
        if (n > kMaShort) ma_rank_sort(vf_raw + s, vf + s, n, (int)threadIdx.x, kImeshThreads);
        if (2 * n > kMaShort) ma_rank_sort(nb_raw + 2 * s, nb_sorted + 2 * s, 2 * n, (int)threadIdx.x, kImeshThreads);
    }
}

// The walk over a vertex's sorted edges: runs of equal neighbour ids.  COUNT: deg[v] = the runs.  FILL: the entries, the flags,
// the statistics of the edges seen from their lower end.
template <bool FILL>
__global__ __launch_bounds__(kImeshThreads) void k_ma_nbr(const int* __restrict__ vf_start, int n_verts, const unsigned* __restrict__ nb_sorted,
                                                          int* __restrict__ deg, const int* __restrict__ nbr_start, int* __restrict__ nbr,
                                                          int* __restrict__ nbr_out, int* __restrict__ nbr_in,
                                                          unsigned char* __restrict__ vert_flags, int* counts) {
    const long long step = (long long)gridDim.x * blockDim.x, end = ((long long)n_verts + 63) & ~63ll;
    int n_edges = 0, n_bound = 0, n_nonman = 0, n_misor = 0, n_isol = 0, most = 0;
    // terminates: end - v strictly decreases (step >= 1) and the loop ends when it reaches 0; the vertex count is rounded up to
    // whole waves so that every lane reaches the reductions below
    for (long long v = (long long)blockIdx.x * blockDim.x + threadIdx.x; v < end; v += step) {
        if (v >= n_verts) continue;
        long long i = 2 * (long long)vf_start[v];
        const long long last = 2 * (long long)vf_start[v + 1];
        long long at = FILL ? nbr_start[v] : 0;
        int runs = 0;
        unsigned flags = 0u;
        while (i < last) {   // terminates: the inner loop advances i at least once (its first test holds: nb_sorted[i] >> 1 == n)
            const unsigned n = nb_sorted[i] >> 1;
            int n_out = 0, n_in = 0;
            while (i < last && (nb_sorted[i] >> 1) == n) {   // terminates: last - i strictly decreases
                if (nb_sorted[i] & 1u) ++n_in; else ++n_out;
                ++i;
            }
            ++runs;
            if constexpr (FILL) {   // at < nbr_start[v + 1] <= 6 F: the COUNT pass counted the same runs
                nbr[at] = (int)n;
                nbr_out[at] = n_out;
                nbr_in[at] = n_in;
                ++at;
                const int tot = n_out + n_in;
                flags |= (tot == 1 ? 1u : 0u) | (tot >= 3 ? 2u : 0u);
                if ((long long)n > v) {
                    ++n_edges;
                    n_bound += tot == 1;
                    n_nonman += tot >= 3;
                    n_misor += tot == 2 && n_out != 1;
                }
            }
        }
        if constexpr (FILL) {
            vert_flags[v] = (unsigned char)(flags | (runs == 0 ? 4u : 0u));
            n_isol += runs == 0;
            most = max(most, runs);
        } else {
            deg[v] = runs;
        }
    }
    if constexpr (FILL) {
        // every lane of every wave is here (no early return above): sums and a maximum over the wave, then one atomic each
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            n_edges += __shfl_down(n_edges, o);
            n_bound += __shfl_down(n_bound, o);
            n_nonman += __shfl_down(n_nonman, o);
            n_misor += __shfl_down(n_misor, o);
            n_isol += __shfl_down(n_isol, o);
            most = max(most, __shfl_down(most, o));
        }
        if ((threadIdx.x & 63) == 0) {
            if (n_edges) atomicAdd(&counts[1], n_edges);
            if (n_bound) atomicAdd(&counts[2], n_bound);
            if (n_nonman) atomicAdd(&counts[3], n_nonman);
            if (n_misor) atomicAdd(&counts[4], n_misor);
            if (most) atomicMax(&counts[5], most);
            if (n_isol) atomicAdd(&counts[6], n_isol);
        }
    }
}

__global__ void k_ma_finish(int* __restrict__ counts, int n_verts) {
    if (blockIdx.x == 0 && threadIdx.x == 0) counts[7] = (n_verts - counts[6]) - counts[1] + counts[0];
}

// ---- per-vertex normals: a gather over vf ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kImeshThreads) void k_ma_normals(const float* __restrict__ verts, int n_verts, const int* __restrict__ faces,
                                                              int n_faces, const int* __restrict__ vf_start, const int* __restrict__ vf,
                                                              double* __restrict__ normal_sum, float* __restrict__ normals) {
#pragma clang fp contract(off)
    const long long step = (long long)gridDim.x * blockDim.x;
    // terminates: n_verts - v strictly decreases (step >= 1) and the loop ends when it reaches 0
    for (long long v = (long long)blockIdx.x * blockDim.x + threadIdx.x; v < n_verts; v += step) {
        double acc[3] = {0.0, 0.0, 0.0};
        // vf_start is the caller's too: clamped to the rows vf has
        const long long last = min((long long)vf_start[v + 1], 3 * (long long)n_faces);
        for (long long i = max(vf_start[v], 0); i < last; ++i) {   // terminates: last - i strictly decreases
            const int f = vf[i];
            int id[3];
            // vf is the caller's: a row that names no valid face of THIS mesh is skipped instead of followed out of bounds
            if ((unsigned)f >= (unsigned)n_faces || !ma_face_ok(faces, f, n_verts, id)) continue;
            double p[3][3];
            bool finite = true;
#pragma unroll
            for (int c = 0; c < 3; ++c)
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    const float x = verts[3 * (size_t)id[c] + a];
                    finite = finite && isfinite(x);
                    p[c][a] = (double)x;
                }
            if (!finite) continue;
            const double ax = p[1][0] - p[0][0], ay = p[1][1] - p[0][1], az = p[1][2] - p[0][2];
            const double bx = p[2][0] - p[0][0], by = p[2][1] - p[0][1], bz = p[2][2] - p[0][2];
            acc[0] = acc[0] + (ay * bz - az * by);
            acc[1] = acc[1] + (az * bx - ax * bz);
            acc[2] = acc[2] + (ax * by - ay * bx);
        }
        const double len = sqrt((acc[0] * acc[0] + acc[1] * acc[1]) + acc[2] * acc[2]);
        const bool ok = isfinite(len) && len > 0.0;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            normal_sum[3 * v + a] = acc[a];
            normals[3 * v + a] = ok ? (float)(acc[a] / len) : 0.0f;
        }
    }
}

// ---- one smoothing step: a gather over nbr -----------------------------------------------------------------------------------------
__global__ __launch_bounds__(kImeshThreads) void k_ma_smooth(const float* __restrict__ src, int n_verts, const int* __restrict__ nbr_start,
                                                             const int* __restrict__ nbr, const unsigned char* __restrict__ vert_flags,
                                                             double factor, int pin, float* __restrict__ dst) {
#pragma clang fp contract(off)
    const long long step = (long long)gridDim.x * blockDim.x;
    // terminates: n_verts - v strictly decreases (step >= 1) and the loop ends when it reaches 0
    for (long long v = (long long)blockIdx.x * blockDim.x + threadIdx.x; v < n_verts; v += step) {
        const float p[3] = {src[3 * v + 0], src[3 * v + 1], src[3 * v + 2]};
        float out[3] = {p[0], p[1], p[2]};
        const bool free_to_move = isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]) && !(pin && (vert_flags[v] & 3));
        if (free_to_move) {
            double s[3] = {0.0, 0.0, 0.0};
            int m = 0;
            const long long last = nbr_start[v + 1];
            for (long long i = nbr_start[v]; i < last; ++i) {   // terminates: last - i strictly decreases
                const int n = nbr[i];
                if ((unsigned)n >= (unsigned)n_verts) continue;   // nbr is the caller's: never followed out of bounds
                const float q[3] = {src[3 * (size_t)n + 0], src[3 * (size_t)n + 1], src[3 * (size_t)n + 2]};
                if (!(isfinite(q[0]) && isfinite(q[1]) && isfinite(q[2]))) continue;
                s[0] = s[0] + (double)q[0];
                s[1] = s[1] + (double)q[1];
                s[2] = s[2] + (double)q[2];
                ++m;
            }
            if (m > 0) {
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    const double pa = (double)p[a];
                    out[a] = (float)(pa + factor * (s[a] / (double)m - pa));
                }
            }
        }
        dst[3 * v + 0] = out[0];
        dst[3 * v + 1] = out[1];
        dst[3 * v + 2] = out[2];
    }
}

// ---- one step of tangential relaxation: k_ma_smooth's gather, the move without its part along the vertex normal ----------------
// A vertex moves when it is finite, not on a boundary or non-manifold edge, has a finite neighbour, and nn = (N0 N0 + N1 N1) +
// N2 N2 of its normal_sum N (arah_mesh_vertex_normals' double output) is finite and > 0: d = s / m - p as above, t = ((d0 N0 +
// d1 N1) + d2 N2) / nn, new = float(p + factor (d - t N)).  No square root.  meshing.mesh_tangential_step is the rule.
__global__ __launch_bounds__(kImeshThreads) void k_ma_tangential(const float* __restrict__ src, int n_verts, const int* __restrict__ nbr_start,
                                                                 const int* __restrict__ nbr, const unsigned char* __restrict__ vert_flags,
                                                                 const double* __restrict__ normal_sum, double factor,
                                                                 float* __restrict__ dst) {
#pragma clang fp contract(off)
    const long long step = (long long)gridDim.x * blockDim.x;
    // terminates: n_verts - v strictly decreases (step >= 1) and the loop ends when it reaches 0
    for (long long v = (long long)blockIdx.x * blockDim.x + threadIdx.x; v < n_verts; v += step) {
        const float p[3] = {src[3 * v + 0], src[3 * v + 1], src[3 * v + 2]};
        float out[3] = {p[0], p[1], p[2]};
        const double N[3] = {normal_sum[3 * v + 0], normal_sum[3 * v + 1], normal_sum[3 * v + 2]};
        const double nn = (N[0] * N[0] + N[1] * N[1]) + N[2] * N[2];
        if (isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]) && !(vert_flags[v] & 3) && isfinite(nn) && nn > 0.0) {
            double s[3] = {0.0, 0.0, 0.0};
            int m = 0;
            const long long last = nbr_start[v + 1];
            for (long long i = nbr_start[v]; i < last; ++i) {   // terminates: last - i strictly decreases
                const int n = nbr[i];
                if ((unsigned)n >= (unsigned)n_verts) continue;   // nbr is the caller's: never followed out of bounds
                const float q[3] = {src[3 * (size_t)n + 0], src[3 * (size_t)n + 1], src[3 * (size_t)n + 2]};
                if (!(isfinite(q[0]) && isfinite(q[1]) && isfinite(q[2]))) continue;
                s[0] = s[0] + (double)q[0];
                s[1] = s[1] + (double)q[1];
                s[2] = s[2] + (double)q[2];
                ++m;
            }
            if (m > 0) {
                double d[3];
#pragma unroll
                for (int a = 0; a < 3; ++a) d[a] = s[a] / (double)m - (double)p[a];
                const double t = ((d[0] * N[0] + d[1] * N[1]) + d[2] * N[2]) / nn;
#pragma unroll
                for (int a = 0; a < 3; ++a) out[a] = (float)((double)p[a] + factor * (d[a] - t * N[a]));
            }
        }
        dst[3 * v + 0] = out[0];
        dst[3 * v + 1] = out[1];
        dst[3 * v + 2] = out[2];
    }
}

__global__ __launch_bounds__(kImeshThreads) void k_ma_copy(const float* __restrict__ src, long long n, float* __restrict__ dst) {
    const long long step = (long long)gridDim.x * blockDim.x;
    // terminates: n - i strictly decreases (step >= 1) and the loop ends when it reaches 0
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += step) dst[i] = src[i];
}
