// meshlaplace.hpp -- the cotangent Laplacian of an indexed mesh on the device, and what stands on it: the operator applied to
// per-vertex values, mean / Gaussian / principal curvatures, and umbrella smoothing with cotangent weights.
//
// Reference: none in its tree (its users take these from trimesh / libigl / pytorch3d; none is a dependency of this project).
// The rule is meshing.mesh_cotangent / laplacian_apply / mesh_curvature / mesh_smooth(weights="cotangent"), restated here once:
//
//   * a valid face (meshadj.hpp) with corners p0, p1, p2 widened to float64 is NONFINITE when a coordinate is not finite;
//     otherwise N = (p1 - p0) x (p2 - p0) as k_ma_normals forms it, A2 = sqrt((N0 N0 + N1 N1) + N2 N2), and the face is DEGENERATE
//     when A2 is 0 or not finite.  Both kinds contribute nothing.  For corner c with u, w the edges leaving it to the next and the
//     previous corner: dot_c = (u0 w0 + u1 w1) + u2 w2, cot_c = dot_c / A2, angle_c = atan2(A2, dot_c), l2_c = the squared length
//     of the opposite edge e = p[c + 2] - p[c + 1], (e0 e0 + e1 e1) + e2 e2;
//   * weight of the neighbour entry (v, n) = 0.5 * the sum of cot(corner opposite {v, n}) over the contributing faces that hold both,
//     in ASCENDING FACE ID, from 0: a per-face quantity summed in an order both ends share, so (v, n) and (n, v) carry the same bits;
//   * diag[v] = the sum of its entries' weights in ascending neighbour id; angle_sum[v] = the sum of angle at v over its contributing
//     faces in ascending face id; area[v]: mass 0 (barycentric) (sum of A2) / 6; mass 1 (mixed, Meyer et al. 2002) the sum of the
//     face's share: no corner with dot < 0: (l2_a cot_a + l2_b cot_b) 0.125 with a, b the other two corners; otherwise, with o the
//     FIRST corner of the face with dot < 0, A2 0.25 for o and A2 0.125 for the other two;
//   * counts[0 .. 5]: contributing, degenerate, nonfinite faces, contributing faces with a corner dot < 0, entries with n > v and
//     weight < 0, vertices whose area is not > 0; counts[6], counts[7] = 0.
//
// arah_mesh_cotangent, one launch per line (after two memsets: weight = +0.0 everywhere, counts = 0):
//
//   k_ml_cot_short   one thread per vertex with at most kMaShort incident faces: ONE walk over its faces in ascending id; each face
//                    is evaluated once, its angle and area share are added, and the cotangents opposite to its two edges at v are
//                    added to the vertex's OWN entries (found by bisection in its sorted row).  Then the row is halved and summed.
//                    A face counts once, at its first corner.
//   k_ml_cot_long    one workgroup per vertex with more incident faces (a fan's apex): the entries are spread over the threads,
//                    each walks the face row for the faces that hold its neighbour (n^2 / 256 id tests per thread instead of n
//                    bisections behind n serial face evaluations in one lane); after a barrier thread 0 walks the faces once for
//                    the angle and the area and sums the row.
//
// A gather throughout: a vertex's own lane, or its workgroup, writes that vertex's entries, and every sum is a loop in a stated
// order -- the order of arrival does not show.  Integer atomics for the counters only.  vf_start / vf / nbr_start / nbr are the
// caller's: rows are clamped to the arrays, ids are tested before they are followed.  No thread waits for another beyond
// __syncthreads from workgroup-uniform control flow; every loop ends by an argument of its own, stated at the loop.
// `#pragma clang fp contract(off)` stands in EVERY function that does arithmetic: it does not reach an inlined helper.
// The clamp of a vertex's rows (ma_segment) and ma_dot are meshedge.hpp's.
#pragma once

constexpr double kMlTwoPi = 6.283185307179586;    // the doubles nearest to 2 pi and pi: meshing.TWO_PI, meshing.PI
constexpr double kMlPi = 3.141592653589793;
constexpr int kMlMaxChannels = 32;                 // columns of x in arah_mesh_laplacian_apply
constexpr int kMlCounts = 8;

struct MlFace {
    double A2, dot[3], l2[3];
    int state;   // 0 contributing, 1 degenerate, 2 nonfinite
};

// the face with the valid ids `id` (all < n_verts: ma_face_ok)
__device__ __forceinline__ void ml_face(const float* __restrict__ verts, const int id[3], MlFace& t) {
#pragma clang fp contract(off)
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
    t.state = 2;
    if (!finite) return;
    const double ax = p[1][0] - p[0][0], ay = p[1][1] - p[0][1], az = p[1][2] - p[0][2];
    const double bx = p[2][0] - p[0][0], by = p[2][1] - p[0][1], bz = p[2][2] - p[0][2];
    const double N[3] = {ay * bz - az * by, az * bx - ax * bz, ax * by - ay * bx};
    t.A2 = sqrt(ma_dot(N, N));
    t.state = 1;
    if (!(isfinite(t.A2) && t.A2 > 0.0)) return;
    t.state = 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int a = (c + 1) % 3, b = (c + 2) % 3;
        const double u[3] = {p[a][0] - p[c][0], p[a][1] - p[c][1], p[a][2] - p[c][2]};
        const double w[3] = {p[b][0] - p[c][0], p[b][1] - p[c][1], p[b][2] - p[c][2]};
        const double e[3] = {p[b][0] - p[a][0], p[b][1] - p[a][1], p[b][2] - p[a][2]};
        t.dot[c] = ma_dot(u, w);
        t.l2[c] = ma_dot(e, e);
    }
}

// x[i] for a corner i known at run time only, by selects: an indexed read would put the face into scratch memory
__device__ __forceinline__ double ml_at(const double* x, int i) { return i == 0 ? x[0] : i == 1 ? x[1] : x[2]; }

// the first corner with dot < 0, or -1
__device__ __forceinline__ int ml_obtuse(const MlFace& t) { return t.dot[0] < 0.0 ? 0 : t.dot[1] < 0.0 ? 1 : t.dot[2] < 0.0 ? 2 : -1; }

// corner c's share of the face's area: mass 0 the doubled area itself (the vertex divides its sum by 6), mass 1 the mixed cell
__device__ __forceinline__ double ml_share(const MlFace& t, int c, int mass) {
#pragma clang fp contract(off)
    if (mass == 0) return t.A2;
    const int o = ml_obtuse(t);
    if (o >= 0) return o == c ? t.A2 * 0.25 : t.A2 * 0.125;
    const int a = (c + 1) % 3, b = (c + 2) % 3;
    return (ml_at(t.l2, a) * (ml_at(t.dot, a) / t.A2) + ml_at(t.l2, b) * (ml_at(t.dot, b) / t.A2)) * 0.125;
}

// the row of `key` in the ascending ids nbr[lo .. hi), or -1; leaves at the first equal row (meshedge.hpp's ma_lower does not)
__device__ __forceinline__ long long ml_find(const int* __restrict__ nbr, long long lo, long long hi, int key) {
    while (lo < hi) {   // terminates: hi - lo at least halves
        const long long mid = lo + ((hi - lo) >> 1);
        const int x = nbr[mid];
        if (x == key) return mid;
        if (x < key) lo = mid + 1; else hi = mid;
    }
    return -1;
}

struct MlRows {
    long long fs, fe, es, ee;   // the vertex's rows of vf and of nbr, clamped to the arrays
};

__device__ __forceinline__ MlRows ml_rows(const int* __restrict__ vf_start, const int* __restrict__ nbr_start, long long v, int n_faces) {
    MlRows r;
    ma_segment(vf_start, v, 3ll * n_faces, r.fs, r.fe);
    ma_segment(nbr_start, v, 6ll * n_faces, r.es, r.ee);
    return r;
}

struct MlTally {
    int used, degenerate, nonfinite, obtuse, negative, bad_area;
};

// The walk over the faces of v in ascending id.  WEIGHTS: the cotangents are added to the (zeroed) rows of v's entries.  FULL: the
// angle and the area sums.  A face is tallied at its first corner.
template <bool FULL, bool WEIGHTS>
__device__ __forceinline__ void ml_walk_faces(const float* __restrict__ verts, int n_verts, const int* __restrict__ faces, int n_faces,
                                              const int* __restrict__ vf, const int* __restrict__ nbr, const MlRows& r, int v, int mass,
                                              double* weight, double& ang, double& ar, MlTally& tally) {
#pragma clang fp contract(off)
    for (long long i = r.fs; i < r.fe; ++i) {   // terminates: fe - i strictly decreases
        const int f = vf[i];
        int id[3];
        if ((unsigned)f >= (unsigned)n_faces || !ma_face_ok(faces, f, n_verts, id)) continue;
        const int c = id[0] == v ? 0 : id[1] == v ? 1 : id[2] == v ? 2 : -1;
        if (c < 0) continue;
        MlFace t;
        ml_face(verts, id, t);
        if (c == 0) {
            tally.used += t.state == 0;
            tally.degenerate += t.state == 1;
            tally.nonfinite += t.state == 2;
            tally.obtuse += t.state == 0 && ml_obtuse(t) >= 0;
        }
        if (t.state) continue;
        if constexpr (FULL) {
            ang = ang + atan2(t.A2, ml_at(t.dot, c));
            ar = ar + ml_share(t, c, mass);
        }
        if constexpr (WEIGHTS) {
            const int a = (c + 1) % 3, b = (c + 2) % 3;
            const int na = a == 0 ? id[0] : a == 1 ? id[1] : id[2], nb = b == 0 ? id[0] : b == 1 ? id[1] : id[2];
            const long long ia = ml_find(nbr, r.es, r.ee, na), ib = ml_find(nbr, r.es, r.ee, nb);
            if (ia >= 0) weight[ia] = weight[ia] + ml_at(t.dot, b) / t.A2;   // the edge {v, na} lies opposite to corner b
            if (ib >= 0) weight[ib] = weight[ib] + ml_at(t.dot, a) / t.A2;
        }
    }
}

// the row of sums halved in place and summed in ascending neighbour id; the outputs of the vertex
template <bool FULL>
__device__ __forceinline__ void ml_finish_vertex(const int* __restrict__ nbr, const MlRows& r, int v, int mass, double ang, double ar,
                                                 double* weight, double* __restrict__ diag, double* __restrict__ area,
                                                 double* __restrict__ angle_sum, MlTally& tally) {
#pragma clang fp contract(off)
    double d = 0.0;
    for (long long i = r.es; i < r.ee; ++i) {   // terminates: ee - i strictly decreases
        const double w = 0.5 * weight[i];
        weight[i] = w;
        d = d + w;
        tally.negative += nbr[i] > v && w < 0.0;
    }
    if constexpr (FULL) {
        const double a = mass == 0 ? ar / 6.0 : ar;
        diag[v] = d;
        area[v] = a;
        angle_sum[v] = ang;
        tally.bad_area += !(a > 0.0);
    }
}

template <bool FULL>
__global__ __launch_bounds__(kImeshThreads) void k_ml_cot_short(const float* __restrict__ verts, int n_verts, const int* __restrict__ faces,
                                                                int n_faces, const int* __restrict__ vf_start, const int* __restrict__ vf,
                                                                const int* __restrict__ nbr_start, const int* __restrict__ nbr, int mass,
                                                                double* weight, double* __restrict__ diag, double* __restrict__ area,
                                                                double* __restrict__ angle_sum, int* counts) {
    const long long step = (long long)gridDim.x * blockDim.x, end = ((long long)n_verts + 63) & ~63ll;
    MlTally tally{};
    // terminates: end - v strictly decreases (step >= 1) and the loop ends when it reaches 0; the vertex count is rounded up to
    // whole waves so that every lane reaches the reductions below
    for (long long v = (long long)blockIdx.x * blockDim.x + threadIdx.x; v < end; v += step) {
        if (v >= n_verts) continue;
        const MlRows r = ml_rows(vf_start, nbr_start, v, n_faces);
        if (r.fe - r.fs > kMaShort) continue;   // k_ml_cot_long's
        double ang = 0.0, ar = 0.0;
        ml_walk_faces<FULL, true>(verts, n_verts, faces, n_faces, vf, nbr, r, (int)v, mass, weight, ang, ar, tally);
        ml_finish_vertex<FULL>(nbr, r, (int)v, mass, ang, ar, weight, diag, area, angle_sum, tally);
    }
    int part[6] = {tally.used, tally.degenerate, tally.nonfinite, tally.obtuse, tally.negative, tally.bad_area};
#pragma unroll
    for (int k = 0; k < 6; ++k) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) part[k] += __shfl_down(part[k], o);
        if ((threadIdx.x & 63) == 0 && part[k]) atomicAdd(&counts[k], part[k]);
    }
}

template <bool FULL>
__global__ __launch_bounds__(kImeshThreads) void k_ml_cot_long(const float* __restrict__ verts, int n_verts, const int* __restrict__ faces,
                                                               int n_faces, const int* __restrict__ vf_start, const int* __restrict__ vf,
                                                               const int* __restrict__ nbr_start, const int* __restrict__ nbr, int mass,
                                                               double* weight, double* __restrict__ diag, double* __restrict__ area,
                                                               double* __restrict__ angle_sum, int* counts) {
#pragma clang fp contract(off)
    // terminates: n_verts - v strictly decreases (gridDim.x >= 1).  v and its rows are the same for every thread of the workgroup,
    // so the barrier is reached by all of them or by none
    for (long long v = blockIdx.x; v < n_verts; v += gridDim.x) {
        const MlRows r = ml_rows(vf_start, nbr_start, v, n_faces);
        if (r.fe - r.fs <= kMaShort) continue;   // k_ml_cot_short's
        for (long long i = r.es + threadIdx.x; i < r.ee; i += kImeshThreads) {   // terminates: ee - i strictly decreases
            const int n = nbr[i];
            double acc = 0.0;
            if ((unsigned)n < (unsigned)n_verts && n != (int)v) {
                for (long long j = r.fs; j < r.fe; ++j) {   // terminates: fe - j strictly decreases
                    const int f = vf[j];
                    int id[3];
                    if ((unsigned)f >= (unsigned)n_faces || !ma_face_ok(faces, f, n_verts, id)) continue;
                    const int cv = id[0] == (int)v ? 0 : id[1] == (int)v ? 1 : id[2] == (int)v ? 2 : -1;
                    const int cn = id[0] == n ? 0 : id[1] == n ? 1 : id[2] == n ? 2 : -1;
                    if (cv < 0 || cn < 0) continue;
                    MlFace t;
                    ml_face(verts, id, t);
                    if (t.state) continue;
                    acc = acc + ml_at(t.dot, 3 - cv - cn) / t.A2;
                }
            }
            weight[i] = acc;
        }
        __syncthreads();   // the row of sums is complete, and visible to thread 0
        if (threadIdx.x == 0) {
            MlTally tally{};
            double ang = 0.0, ar = 0.0;
            ml_walk_faces<FULL, false>(verts, n_verts, faces, n_faces, vf, nbr, r, (int)v, mass, weight, ang, ar, tally);
            ml_finish_vertex<FULL>(nbr, r, (int)v, mass, ang, ar, weight, diag, area, angle_sum, tally);
            const int part[6] = {tally.used, tally.degenerate, tally.nonfinite, tally.obtuse, tally.negative, tally.bad_area};
            for (int k = 0; k < 6; ++k)
                if (part[k]) atomicAdd(&counts[k], part[k]);
        }
    }
}

// ---- y = L x: one thread per (vertex, column) -----------------------------------------------------------------------------------
// y[v][c] = the sum over v's entries in ascending neighbour id, from 0, of weight (x[n][c] - x[v][c]) in float64; an entry whose
// weight or x[n][c] is not finite is skipped; where x[v][c] itself is not finite y is THE quiet NaN 0x7ff8000000000000 (the bits of
// an arithmetic NaN are the hardware's own).  Neighbouring lanes read the same row of weights and neighbouring columns of x.
template <class T>
__global__ __launch_bounds__(kImeshThreads) void k_ml_apply(const double* __restrict__ weight, const int* __restrict__ nbr_start,
                                                            const int* __restrict__ nbr, int n_verts, long long n_rows,
                                                            const T* __restrict__ x, int n_ch, double* __restrict__ y) {
#pragma clang fp contract(off)
    const long long step = (long long)gridDim.x * blockDim.x, total = (long long)n_verts * n_ch;
    // terminates: total - i strictly decreases (step >= 1)
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += step) {
        const long long v = i / n_ch;
        const int c = (int)(i - v * n_ch);
        const double xv = (double)x[i];
        long long es, ee;
        ma_segment(nbr_start, v, n_rows, es, ee);
        double acc = 0.0;
        for (long long k = es; k < ee; ++k) {   // terminates: ee - k strictly decreases
            const int n = nbr[k];
            if ((unsigned)n >= (unsigned)n_verts) continue;   // nbr is the caller's: never followed out of bounds
            const double w = weight[k], xn = (double)x[(size_t)n * n_ch + c];
            if (!(isfinite(w) && isfinite(xn))) continue;
            acc = acc + w * (xn - xv);
        }
        y[i] = isfinite(xv) ? acc : __longlong_as_double(0x7ff8000000000000ll);
    }
}

// ---- curvatures: one thread per vertex --------------------------------------------------------------------------------------------
// L = k_ml_apply's sum over the positions; K = (-L) / area (Meyer's 2 kappa_H n); mean_normal = 0.5 K; mean_abs = 0.5 sqrt(K.K);
// mean = 0.5 ((K.N) / sqrt(N.N)) with N = normal_sum; gaussian = ((2 pi, or pi with vert_flags bit 0) - angle_sum) / area; r =
// sqrt(max(mean mean - gaussian, 0)), k1 = mean + r, k2 = mean - r.  INVALID -- NaN everywhere, valid = 0, counted: bit 1 or 2 of
// vert_flags, a non-finite coordinate, area not finite and > 0, sqrt(N.N) not finite and > 0.  curv rows: mean, mean_abs, gaussian,
// k1, k2.
__global__ __launch_bounds__(kImeshThreads) void k_ml_curvature(const float* __restrict__ verts, int n_verts, const int* __restrict__ nbr_start,
                                                                const int* __restrict__ nbr, long long n_rows,
                                                                const unsigned char* __restrict__ vert_flags,
                                                                const double* __restrict__ weight, const double* __restrict__ area,
                                                                const double* __restrict__ angle_sum, const double* __restrict__ normal_sum,
                                                                double* __restrict__ curv, double* __restrict__ mean_normal,
                                                                unsigned char* __restrict__ valid, int* counts) {
#pragma clang fp contract(off)
    const long long step = (long long)gridDim.x * blockDim.x, end = ((long long)n_verts + 63) & ~63ll;
    int n_invalid = 0;
    // terminates: end - v strictly decreases (step >= 1); whole waves reach the reduction below
    for (long long v = (long long)blockIdx.x * blockDim.x + threadIdx.x; v < end; v += step) {
        if (v >= n_verts) continue;
        const float pf[3] = {verts[3 * v + 0], verts[3 * v + 1], verts[3 * v + 2]};
        const double N[3] = {normal_sum[3 * v + 0], normal_sum[3 * v + 1], normal_sum[3 * v + 2]};
        const double a = area[v], len = sqrt(ma_dot(N, N));
        const unsigned flags = vert_flags[v];
        const bool ok = !(flags & 6u) && isfinite(pf[0]) && isfinite(pf[1]) && isfinite(pf[2]) && isfinite(a) && a > 0.0 && isfinite(len) &&
                        len > 0.0;
        const double nan = __longlong_as_double(0x7ff8000000000000ll);
        double out[5] = {nan, nan, nan, nan, nan}, mn[3] = {nan, nan, nan};
        if (ok) {
            const double p[3] = {(double)pf[0], (double)pf[1], (double)pf[2]};
            double L[3] = {0.0, 0.0, 0.0};
            long long es, ee;
            ma_segment(nbr_start, v, n_rows, es, ee);
            for (long long k = es; k < ee; ++k) {   // terminates: ee - k strictly decreases
                const int n = nbr[k];
                if ((unsigned)n >= (unsigned)n_verts) continue;   // nbr is the caller's: never followed out of bounds
                const double w = weight[k];
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const double q = (double)verts[3 * (size_t)n + c];
                    if (isfinite(w) && isfinite(q)) L[c] = L[c] + w * (q - p[c]);
                }
            }
            const double K[3] = {(-L[0]) / a, (-L[1]) / a, (-L[2]) / a};
            const double mean = 0.5 * (ma_dot(K, N) / len);
            const double gauss = (((flags & 1u) ? kMlPi : kMlTwoPi) - angle_sum[v]) / a;
            const double disc = mean * mean - gauss;
            const double root = sqrt(disc > 0.0 ? disc : 0.0);
            out[0] = mean;
            out[1] = 0.5 * sqrt(ma_dot(K, K));
            out[2] = gauss;
            out[3] = mean + root;
            out[4] = mean - root;
#pragma unroll
            for (int c = 0; c < 3; ++c) mn[c] = 0.5 * K[c];
        }
#pragma unroll
        for (int k = 0; k < 5; ++k) curv[5 * v + k] = out[k];
#pragma unroll
        for (int c = 0; c < 3; ++c) mean_normal[3 * v + c] = mn[c];
        valid[v] = ok ? 1 : 0;
        n_invalid += !ok;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) n_invalid += __shfl_down(n_invalid, o);
    if ((threadIdx.x & 63) == 0 && n_invalid) atomicAdd(&counts[0], n_invalid);
}

// ---- one smoothing step with cotangent weights: k_ma_smooth's gather with the weights of this step's positions --------------------
// A vertex moves when it is finite, is not pinned, and s = the sum of |w| over its entries with a finite neighbour and a finite w,
// in ascending id, is finite and > 0: acc = the sum of w (q - p) over the same entries with the weights' own signs, new = float(p +
// factor (acc / s)).  The signed sum is what vanishes on a flat patch; |w| in the denominator keeps the step inside the 1-ring.
__global__ __launch_bounds__(kImeshThreads) void k_ml_smooth(const float* __restrict__ src, int n_verts, const int* __restrict__ nbr_start,
                                                             const int* __restrict__ nbr, long long n_rows,
                                                             const unsigned char* __restrict__ vert_flags, const double* __restrict__ weight,
                                                             double factor, int pin, float* __restrict__ dst) {
#pragma clang fp contract(off)
    const long long step = (long long)gridDim.x * blockDim.x;
    // terminates: n_verts - v strictly decreases (step >= 1) and the loop ends when it reaches 0
    for (long long v = (long long)blockIdx.x * blockDim.x + threadIdx.x; v < n_verts; v += step) {
        const float p[3] = {src[3 * v + 0], src[3 * v + 1], src[3 * v + 2]};
        float out[3] = {p[0], p[1], p[2]};
        if (isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]) && !(pin && (vert_flags[v] & 3))) {
            double acc[3] = {0.0, 0.0, 0.0}, s = 0.0;
            long long es, ee;
            ma_segment(nbr_start, v, n_rows, es, ee);
            for (long long i = es; i < ee; ++i) {   // terminates: ee - i strictly decreases
                const int n = nbr[i];
                if ((unsigned)n >= (unsigned)n_verts) continue;   // nbr is the caller's: never followed out of bounds
                const double w = weight[i];
                if (!isfinite(w)) continue;
                const float q[3] = {src[3 * (size_t)n + 0], src[3 * (size_t)n + 1], src[3 * (size_t)n + 2]};
                if (!(isfinite(q[0]) && isfinite(q[1]) && isfinite(q[2]))) continue;
                s = s + fabs(w);
#pragma unroll
                for (int a = 0; a < 3; ++a) acc[a] = acc[a] + w * ((double)q[a] - (double)p[a]);
            }
            if (isfinite(s) && s > 0.0) {
#pragma unroll
                for (int a = 0; a < 3; ++a) out[a] = (float)((double)p[a] + factor * (acc[a] / s));
            }
        }
        dst[3 * v + 0] = out[0];
        dst[3 * v + 1] = out[1];
        dst[3 * v + 2] = out[2];
    }
}
