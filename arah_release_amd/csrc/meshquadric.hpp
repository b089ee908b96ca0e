// meshquadric.hpp -- quadric-error placement of the clusters of meshsimp.hpp, on the device.
//
// Reference: none (see meshsimp.hpp).  arah_mesh_simplify puts a cluster at the mean of its members; a mean of points on a convex
// surface lies inside it, so a clustered body shrinks.  Here every cluster moves to the minimiser of Lindstrom's area^2-weighted
// plane quadric of the faces that touch it, taken about its mean and regularised towards it.  The rule is meshing.
// mesh_quadric_place, float64 with every operation rounded on its own and a summation order that is part of the rule, so that the
// result is compared with it bit for bit:
//
//   * a face is valid when its ids lie in [0, V) and vert_map in [0, K) for all three; it contributes once to each distinct
//     cluster of its corners (collapsed and duplicate faces too);
//   * term of face f for cluster k: mq_term below; the terms of a cluster in ASCENDING FACE ID at positions 0 .. n - 1 are summed
//     by the in-place tree "for stride = 1, 2, 4, ... < n: x[i] += x[i + stride] for i a multiple of 2 stride, i + stride < n".
//     Its shape depends on n alone: the last step adds the tree of the first s elements (s the largest power of two below n) and
//     the tree of the rest, and the same holds inside every aligned power-of-two block.  So a lane may run it as a binary
//     counter of partial sums (mq_lane_sum) and a workgroup as the tree over aligned blocks of kImeshThreads terms followed by
//     the same tree over the blocks' sums (k_mq_place_long): equal bits;
//   * solve: mq_solve below; a cluster falls back to its mean, and is counted, when the trace or the determinant is not finite or
//     not positive or a component of the offset is not finite or longer than the cell;
//   * a cluster with more than kMqLimit = 2^15 pairs is not placed: it keeps the mean and sets the status 2 (its segment would be
//     rank-sorted in n^2 steps, and a cell that coarse gains nothing from a quadric);
//   * representative: the member with the smallest float32 d^2 to the NEW position, ties to the lowest id: one 64-bit atomicMin.
//
// arah_mesh_quadric_place, one launch per line:
//
//   k_mq_init         counts of pairs, cursors, packed minima, qcounts: cleared
//   k_mq_count        one thread per face: cnt[cluster] += 1 for its distinct clusters
//   k_mc_scan         start = the exclusive scan of cnt, start[V] = the pairs
//   k_mq_fill         the same walk: raw[start[cluster] + cursor[cluster]++] = f
//   k_mq_sort_short   one thread per cluster of at most kMqShort pairs: ma_rank_sort of its segment (meshadj.hpp)
//   k_mq_sort_long    one workgroup per longer cluster, up to kMqLimit
//   k_mq_place_short  one thread per cluster: the longest segment, the status; at most kMqShort pairs: terms, sum, solve, pos
//   k_mq_place_long   one workgroup per longer cluster: terms and tree in LDS, thread 0 solves
//   k_mq_pick         one thread per vertex: best[cluster] = min of (bits(d^2) << 32) | v
//   k_mq_finish       vert_src; the rows from K on zeroed; qcounts[1] = the pairs
//
// K is read on the device (counts[0], clamped to [0, V]).  Integer atomics only (add, min, max): the cursor decides a layout that
// is sorted afterwards, nothing else depends on the order of arrival.  No thread waits for another: no spin-wait, no grid-wide
// barrier; every loop ends by an argument of its own, stated at the loop.  The two size classes (kMqShort) are unmeasured.
#pragma once

constexpr int kMqShort = 32;                              // pairs of a segment one lane still sorts and sums alone
constexpr int kMqLevels = 6;                              // levels of the lane's counter: 2^(kMqLevels - 1) = kMqShort
constexpr int kMqLimit = 1 << 15;                         // pairs of a segment that is still placed
constexpr int kMqBlocks = kMqLimit / kImeshThreads;       // aligned blocks of a longest segment: their sums fit one more tree
constexpr int kMqLongGrid = 1024;                         // workgroups that share the long segments
constexpr unsigned long long kMqEmpty = ~0ull;
static_assert((1 << (kMqLevels - 1)) == kMqShort && kMqBlocks <= kImeshThreads, "the two size classes of meshquadric.hpp");

__device__ __forceinline__ int mq_clusters(const int* counts, int n_verts) { return min(max(counts[0], 0), n_verts); }

// the distinct clusters of face f in the order of their first corner -> their number, 0 for a face that is not valid
__device__ __forceinline__ int mq_face_clusters(const int* __restrict__ faces, long long f, int n_verts, const int* __restrict__ vert_map,
                                                int n_clusters, int c[3]) {
    int id[3];
    if (!cc_face_ok(faces, f, n_verts, id)) return 0;
    const int c0 = vert_map[id[0]], c1 = vert_map[id[1]], c2 = vert_map[id[2]];
    if ((unsigned)c0 >= (unsigned)n_clusters || (unsigned)c1 >= (unsigned)n_clusters || (unsigned)c2 >= (unsigned)n_clusters) return 0;
    int n = 0;
    c[n++] = c0;
    if (c1 != c0) c[n++] = c1;
    if (c2 != c0 && c2 != c1) c[n++] = c2;
    return n;
}

// the nine numbers of face f about m: A00 A01 A02 A11 A12 A22 b0 b1 b2; NC = 10 (meshcollapse.hpp): and c = d d, the constant of
// the quadric, from the same d.  The face is valid: its ids lie in [0, V)
template <int NC = 9>
__device__ __forceinline__ void mq_term(const float* __restrict__ verts, const int* __restrict__ faces, long long f, const double m[3],
                                        double q[NC]) {
#pragma clang fp contract(off)
    static_assert(NC == 9 || NC == 10, "nine numbers, or ten with the constant");
    double p[3][3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const size_t v = (size_t)faces[3 * f + j];
#pragma unroll
        for (int a = 0; a < 3; ++a) p[j][a] = (double)verts[3 * v + a] - m[a];
    }
    double e1[3], e2[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        e1[a] = p[1][a] - p[0][a];
        e2[a] = p[2][a] - p[0][a];
    }
    const double nx = e1[1] * e2[2] - e1[2] * e2[1];
    const double ny = e1[2] * e2[0] - e1[0] * e2[2];
    const double nz = e1[0] * e2[1] - e1[1] * e2[0];
    const double d = -((nx * p[0][0] + ny * p[0][1]) + nz * p[0][2]);
    q[0] = nx * nx;
    q[1] = nx * ny;
    q[2] = nx * nz;
    q[3] = ny * ny;
    q[4] = ny * nz;
    q[5] = nz * nz;
    q[6] = nx * d;
    q[7] = ny * d;
    q[8] = nz * d;
    if constexpr (NC == 10) q[9] = d * d;
}

// The tree over the n <= kMqShort terms of a segment by one lane: a binary counter of partial sums.  After i + 1 terms level l
// holds the sum of an aligned block of 2^l terms exactly when bit l of i + 1 is set; a new term climbs while it meets one.
// term(i, x) fills the NC numbers of term i; it is called for i = 0 .. n - 1 in that order, once each.
template <int NC, class Term>
__device__ __forceinline__ void mq_lane_tree(int n, Term term, double q[NC]) {
#pragma clang fp contract(off)
    double st[kMqLevels][NC];
#pragma unroll
    for (int l = 0; l < kMqLevels; ++l)
#pragma unroll
        for (int c = 0; c < NC; ++c) st[l][c] = 0.0;
    // terminates: n - i strictly decreases to 0
    for (int i = 0; i < n; ++i) {
        double x[NC];
        term(i, x);
        bool put = false;
#pragma unroll
        for (int l = 0; l < kMqLevels; ++l) {   // i < kMqShort = 2^(kMqLevels - 1): a zero bit of i exists below kMqLevels
            if (put) continue;
            if ((i >> l) & 1) {
#pragma unroll
                for (int c = 0; c < NC; ++c) x[c] = st[l][c] + x[c];
            } else {
#pragma unroll
                for (int c = 0; c < NC; ++c) st[l][c] = x[c];
                put = true;
            }
        }
    }
    bool have = false;
#pragma unroll
    for (int c = 0; c < NC; ++c) q[c] = 0.0;
#pragma unroll
    for (int l = 0; l < kMqLevels; ++l) {   // the blocks of n's binary digits, the shortest (the last) first
        if (!((n >> l) & 1)) continue;
#pragma unroll
        for (int c = 0; c < NC; ++c) q[c] = have ? st[l][c] + q[c] : st[l][c];
        have = true;
    }
}

// the tree over the faces seg[0 .. n) of a cluster about m
__device__ __forceinline__ void mq_lane_sum(const float* __restrict__ verts, const int* __restrict__ faces, const unsigned* __restrict__ seg,
                                            int n, const double m[3], double q[9]) {
    mq_lane_tree<9>(n, [&](int i, double x[9]) { mq_term(verts, faces, (long long)seg[i], m, x); }, q);
}

// the tree over x[.][0 .. m) in LDS, m <= kImeshThreads, by the whole workgroup (from uniform control flow); the sum lands in
// x[.][0].  A step's targets are multiples of 2 stride and its sources are not, so no row is read and written in one step.
// NC: the rows of x that are summed (meshsolve.hpp sums one or two).
template <int NC = 9>
__device__ __forceinline__ void mq_group_tree(double (*x)[kImeshThreads], int m) {
#pragma clang fp contract(off)
    const int tid = (int)threadIdx.x;
    // terminates: stride doubles until it reaches m <= kImeshThreads
    for (int stride = 1; stride < m; stride <<= 1) {
        __syncthreads();
        if ((tid & (2 * stride - 1)) == 0 && tid + stride < m) {
#pragma unroll
            for (int c = 0; c < NC; ++c) x[c][tid] = x[c][tid] + x[c][tid + stride];
        }
    }
    __syncthreads();
}

// y = the minimiser of the regularised quadric about its own origin; false (and y untouched) when the solve falls back.  q holds
// at least the nine numbers of mq_term
__device__ __forceinline__ bool mq_solve_offset(const double* q, double cell, double reg, double y[3]) {
#pragma clang fp contract(off)
    const double t = (q[0] + q[3]) + q[5];
    if (!isfinite(t) || !(t > 0.0)) return false;
    const double lam = reg * t;
    const double M00 = q[0] + lam, M11 = q[3] + lam, M22 = q[5] + lam, M01 = q[1], M02 = q[2], M12 = q[4];
    const double C00 = M11 * M22 - M12 * M12;
    const double C01 = M02 * M12 - M01 * M22;
    const double C02 = M01 * M12 - M02 * M11;
    const double C11 = M00 * M22 - M02 * M02;
    const double C12 = M01 * M02 - M00 * M12;
    const double C22 = M00 * M11 - M01 * M01;
    const double det = (M00 * C00 + M01 * C01) + M02 * C02;
    if (!isfinite(det) || !(det > 0.0)) return false;
    double z[3];
    z[0] = -((C00 * q[6] + C01 * q[7]) + C02 * q[8]) / det;
    z[1] = -((C01 * q[6] + C11 * q[7]) + C12 * q[8]) / det;
    z[2] = -((C02 * q[6] + C12 * q[7]) + C22 * q[8]) / det;
#pragma unroll
    for (int a = 0; a < 3; ++a)
        if (!isfinite(z[a]) || fabs(z[a]) > cell) return false;
#pragma unroll
    for (int a = 0; a < 3; ++a) y[a] = z[a];
    return true;
}

// pos = float32(m + y), y the minimiser of the regularised quadric; false (and pos untouched) when the cluster falls back
__device__ __forceinline__ bool mq_solve(const double q[9], const double m[3], double cell, double reg, float pos[3]) {
#pragma clang fp contract(off)
    double y[3];
    if (!mq_solve_offset(q, cell, reg, y)) return false;
#pragma unroll
    for (int a = 0; a < 3; ++a) pos[a] = (float)(m[a] + y[a]);
    return true;
}

__global__ __launch_bounds__(kImeshThreads) void k_mq_init(int* __restrict__ cnt, int* __restrict__ cursor,
                                                           unsigned long long* __restrict__ best, int n_verts, int* __restrict__ qcounts) {
    const long long step = (long long)gridDim.x * blockDim.x;
    // terminates: n_verts - i strictly decreases (step >= 1) and the loop ends when it reaches 0
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n_verts; i += step) {
        cnt[i] = 0;
        cursor[i] = 0;
        best[i] = kMqEmpty;
    }
    if (blockIdx.x == 0 && threadIdx.x < 4) qcounts[threadIdx.x] = 0;
}

// FILL = false: cnt[cluster] += 1; FILL = true: the face takes the next row of the cluster's segment
template <bool FILL>
__global__ __launch_bounds__(kImeshThreads) void k_mq_pairs(const int* __restrict__ faces, int n_faces, int n_verts,
                                                            const int* __restrict__ vert_map, const int* __restrict__ counts,
                                                            int* cnt, const int* __restrict__ start, unsigned* __restrict__ raw) {
    const int K = mq_clusters(counts, n_verts);
    const long long step = (long long)gridDim.x * blockDim.x;
    // terminates: n_faces - f strictly decreases (step >= 1) and the loop ends when it reaches 0
    for (long long f = (long long)blockIdx.x * blockDim.x + threadIdx.x; f < n_faces; f += step) {
        int c[3];
        const int n = mq_face_clusters(faces, f, n_verts, vert_map, K, c);
        for (int j = 0; j < n; ++j) {   // terminates: n <= 3
            const int at = atomicAdd(&cnt[c[j]], 1);
            // a cluster takes exactly the rows the count pass counted for it: start[c] + at < start[c + 1] <= 3 F
            if constexpr (FILL) raw[(long long)start[c[j]] + at] = (unsigned)f;
        }
    }
}

__global__ __launch_bounds__(kImeshThreads) void k_mq_sort_short(const int* __restrict__ start, const int* __restrict__ cnt, int n_verts,
                                                                 const int* __restrict__ counts, const unsigned* __restrict__ raw,
                                                                 unsigned* __restrict__ seg) {
    const int K = mq_clusters(counts, n_verts);
    const long long step = (long long)gridDim.x * blockDim.x;
    // terminates: K - k strictly decreases (step >= 1) and the loop ends when it reaches 0
    for (long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x; k < K; k += step) {
        const int n = cnt[k];
        if (n <= kMqShort) ma_rank_sort(raw + start[k], seg + start[k], n, 0, 1);
    }
}

__global__ __launch_bounds__(kImeshThreads) void k_mq_sort_long(const int* __restrict__ start, const int* __restrict__ cnt, int n_verts,
                                                                const int* __restrict__ counts, const unsigned* __restrict__ raw,
                                                                unsigned* __restrict__ seg) {
    const int K = mq_clusters(counts, n_verts);
    // terminates: K - k strictly decreases (gridDim.x >= 1) and the loop ends when it reaches 0.  k and n are the same for every
    // thread of the workgroup; nothing is shared between its threads but the read-only source
    for (long long k = blockIdx.x; k < K; k += gridDim.x) {
        const int n = cnt[k];
        if (n > kMqShort && n <= kMqLimit) ma_rank_sort(raw + start[k], seg + start[k], n, (int)threadIdx.x, kImeshThreads);
    }
}

__global__ __launch_bounds__(kImeshThreads) void k_mq_place_short(const float* __restrict__ verts, const int* __restrict__ faces,
                                                                  int n_verts, const int* __restrict__ counts,
                                                                  const float* __restrict__ means, const int* __restrict__ start,
                                                                  const int* __restrict__ cnt, const unsigned* __restrict__ seg,
                                                                  double cell, double reg, float* __restrict__ pos, int* qcounts) {
    const int K = mq_clusters(counts, n_verts);
    const long long step = (long long)gridDim.x * blockDim.x, end = ((long long)K + 63) & ~63ll;
    const int lane = threadIdx.x & 63;
    // terminates: end - k strictly decreases (step >= 1) and the loop ends when it reaches 0.  The cluster count is rounded up to
    // whole waves so that every lane reaches the ballot and the shuffles; lanes beyond the end carry no cluster
    for (long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x; k < end; k += step) {
        const bool in = k < K;
        const int n = in ? cnt[k] : 0;
        bool fell = false;
        if (in && (n <= kMqShort || n > kMqLimit)) {
            const double m[3] = {(double)means[3 * k + 0], (double)means[3 * k + 1], (double)means[3 * k + 2]};
            float p[3] = {means[3 * k + 0], means[3 * k + 1], means[3 * k + 2]};   // the fall-back: the mean's own bits
            if (n <= kMqShort) {
                double q[9];
                mq_lane_sum(verts, faces, seg + start[k], n, m, q);
                fell = !mq_solve(q, m, cell, reg, p);
            }
            pos[3 * k + 0] = p[0];
            pos[3 * k + 1] = p[1];
            pos[3 * k + 2] = p[2];
        }
        int most = n;
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) most = max(most, __shfl_xor(most, o));
        const unsigned long long n_fell = __ballot(fell);
        if (lane == 0) {
            if (most > 0) atomicMax(&qcounts[2], most);
            if (most > kMqLimit) atomicMax(&qcounts[3], 2);
            if (n_fell) atomicAdd(&qcounts[0], (int)__popcll(n_fell));
        }
    }
}

__global__ __launch_bounds__(kImeshThreads) void k_mq_place_long(const float* __restrict__ verts, const int* __restrict__ faces,
                                                                 int n_verts, const int* __restrict__ counts,
                                                                 const float* __restrict__ means, const int* __restrict__ start,
                                                                 const int* __restrict__ cnt, const unsigned* __restrict__ seg,
                                                                 double cell, double reg, float* __restrict__ pos, int* qcounts) {
    __shared__ double x[9][kImeshThreads];
    __shared__ double part[9][kMqBlocks];
    const int K = mq_clusters(counts, n_verts);
    const int tid = (int)threadIdx.x;
    // terminates: K - k strictly decreases (gridDim.x >= 1) and the loop ends when it reaches 0.  k, n and every bound below are
    // the same for every thread of the workgroup, so all of them reach every barrier
    for (long long k = blockIdx.x; k < K; k += gridDim.x) {
        const int n = cnt[k];
        if (n <= kMqShort || n > kMqLimit) continue;
        const unsigned* s = seg + start[k];
        const double m[3] = {(double)means[3 * k + 0], (double)means[3 * k + 1], (double)means[3 * k + 2]};
        const int n_blocks = (n + kImeshThreads - 1) / kImeshThreads;   // <= kMqBlocks
        // terminates: n_blocks - b strictly decreases to 0
        for (int b = 0; b < n_blocks; ++b) {
            const int i = b * kImeshThreads + tid;
            if (i < n) {
                double q[9];
                mq_term(verts, faces, (long long)s[i], m, q);
#pragma unroll
                for (int c = 0; c < 9; ++c) x[c][tid] = q[c];
            }
            mq_group_tree(x, min(kImeshThreads, n - b * kImeshThreads));
            if (tid < 9) part[tid][b] = x[tid][0];
            __syncthreads();   // x is free for the next block, part[.][b] is written
        }
        if (tid < n_blocks) {
#pragma unroll
            for (int c = 0; c < 9; ++c) x[c][tid] = part[c][tid];
        }
        mq_group_tree(x, n_blocks);
        if (tid == 0) {
            double q[9];
#pragma unroll
            for (int c = 0; c < 9; ++c) q[c] = x[c][0];
            float p[3] = {means[3 * k + 0], means[3 * k + 1], means[3 * k + 2]};
            if (!mq_solve(q, m, cell, reg, p)) atomicAdd(&qcounts[0], 1);
            pos[3 * k + 0] = p[0];
            pos[3 * k + 1] = p[1];
            pos[3 * k + 2] = p[2];
        }
        __syncthreads();   // thread 0 has read x before the next cluster writes it
    }
}

__global__ __launch_bounds__(kImeshThreads) void k_mq_pick(const float* __restrict__ verts, int n_verts, const int* __restrict__ vert_map,
                                                           const int* __restrict__ counts, const float* __restrict__ pos,
                                                           unsigned long long* best) {
#pragma clang fp contract(off)
    const int K = mq_clusters(counts, n_verts);
    const long long step = (long long)gridDim.x * blockDim.x;
    // terminates: n_verts - v strictly decreases (step >= 1) and the loop ends when it reaches 0
    for (long long v = (long long)blockIdx.x * blockDim.x + threadIdx.x; v < n_verts; v += step) {
        const int k = vert_map[v];
        if ((unsigned)k >= (unsigned)K) continue;
        const double dx = (double)verts[3 * v + 0] - (double)pos[3 * (size_t)k + 0];
        const double dy = (double)verts[3 * v + 1] - (double)pos[3 * (size_t)k + 1];
        const double dz = (double)verts[3 * v + 2] - (double)pos[3 * (size_t)k + 2];
        const float d2 = (float)((dx * dx + dy * dy) + dz * dz);
        // d2 >= +0 (the sign bit is dropped for a NaN's sake): the bits of a non-negative float order like the float
        atomicMin(&best[k], ((unsigned long long)(__float_as_uint(d2) & 0x7FFFFFFFu) << 32) | (unsigned long long)v);
    }
}

__global__ __launch_bounds__(kImeshThreads) void k_mq_finish(int n_verts, const int* __restrict__ counts, const int* __restrict__ start,
                                                             const unsigned long long* __restrict__ best, float* __restrict__ pos,
                                                             int* __restrict__ vert_src, int* __restrict__ qcounts) {
    const int K = mq_clusters(counts, n_verts);
    if (blockIdx.x == 0 && threadIdx.x == 0) qcounts[1] = start[n_verts];
    const long long step = (long long)gridDim.x * blockDim.x;
    // terminates: n_verts - k strictly decreases (step >= 1) and the loop ends when it reaches 0
    for (long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x; k < n_verts; k += step) {
        if (k < K) {
            vert_src[k] = best[k] == kMqEmpty ? 0 : (int)(best[k] & 0xFFFFFFFFull);   // a member's id lies below n_verts
        } else {
            vert_src[k] = 0;
            pos[3 * k + 0] = 0.f;
            pos[3 * k + 1] = 0.f;
            pos[3 * k + 2] = 0.f;
        }
    }
}

// a mesh without a vertex: no cluster, no pair
__global__ void k_mq_set_empty(int* __restrict__ qcounts) {
    if (blockIdx.x == 0 && threadIdx.x < 4) qcounts[threadIdx.x] = 0;
}
