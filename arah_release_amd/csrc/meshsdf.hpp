// meshsdf.hpp -- the truncated distance field of a triangle soup on a lattice, and its signed value: arah_mesh_sdf_grid.
//
// The rule is meshing.mesh_sdf on the lattice's nodes (meshing.mesh_sdf_grid), and d2 / face equal it bit for bit: per (node,
// triangle) the arithmetic of k_md_closest -- closest_on_triangle, the closest point, d^2, float64 on the float32 data, every
// operation rounded on its own --, per node the lexicographic minimum of (d^2, face id) over the triangles with d^2 <= trunc^2.
//
// It is a SCATTER: the cost follows the band, not the lattice.  One launch per line:
//
//   k_sg_init      d2 <- the bits of +inf, face <- INT_MAX
//   k_sg_setup     one lane per triangle: is it finite (else status 1), the BOX of lattice nodes inside its bounding box dilated by
//                  trunc (a binary search per axis end), and its class by the nodes n of that box: lane (n <= kSgLaneNodes), wave
//                  (<= kSgWaveNodes), workgroup (<= kSgGroupNodes: the MEDIUM list), several workgroups (the HUGE list, kSgParts
//                  parts a triangle) -- the box walkers of meshcommon.hpp (mesh_wave_turns, mesh_list_walk)
//   k_sg_walk<0>, k_sg_walk_lists<0>   every node of every box: d^2; when d^2 <= trunc^2, a 64-bit integer atomicMin on the node's
//                  d2.  Non-negative doubles order like their bit patterns, so this is the exact minimum whatever the arrival order
//   k_sg_walk<1>, k_sg_walk_lists<1>   (only when the face is asked for) the same walk again: a triangle that ATTAINS the node's
//                  minimum does an integer atomicMin of its id on the node's face
//   k_sg_finish    per node: +inf / -1 outside the band, NaN / -1 for a soup with a non-finite vertex or a non-finite node, the
//                  signed value from the occupancy, the band count
//
// Culling is conservative: a node outside a triangle's box is farther than trunc from the triangle's bounding box along some axis
// by more than the slack of sg_axis_range, which covers the rounding of d^2 many times over; inside the box the float64 test
// d^2 <= trunc^2 alone decides.  Integer atomics only, no floating-point atomics; no thread waits for another; every loop ends
// by an argument stated at the loop.  Nothing is truncated: a box of any size is walked whole.  Included by arah_hip.hip after
// meshquery.hpp.
#pragma once

namespace {

constexpr int kSgThreads = 256;
// class thresholds, in nodes of a box: NOT measured.  kSgWaveNodes holds the (3 + 2 + 3)^3 = 512 nodes of a marching-cubes face at
// trunc = 3 steps in the wave class; kSgGroupNodes is 128 nodes a thread
constexpr int kSgLaneNodes = 32;
constexpr int kSgWaveNodes = 2048;
constexpr int kSgGroupNodes = 1 << 15;
constexpr int kSgWaveFaces = 16;   // faces a wave of k_sg_walk holds (see there)
constexpr int kSgParts = 64;
constexpr int kSgListGrid = 2048;
constexpr int kSgMaxGrid = 4096;
constexpr int kSgInfo = 8;   // int32 counters: band nodes, status, tests (uint64 in [2], [3]), triangles lane / wave / group / huge
constexpr unsigned long long kSgInfBits = 0x7ff0000000000000ull;

struct SgScratch {
    int* rect;    // [F][6] i0, i1, j0, j1, k0, k1 (i1 < i0: no node)
    int* med;     // [F]
    int* huge;    // [F]
    size_t bytes;
};

__global__ __launch_bounds__(kSgThreads) void k_sg_init(unsigned long long* __restrict__ d2, int* __restrict__ face, long long n) {
    const long long step = (long long)gridDim.x * blockDim.x;
    // terminates: n - p strictly decreases
    for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += step) {
        d2[p] = kSgInfBits;
        if (face) face[p] = 0x7fffffff;
    }
}

// The nodes i of the ascending axis x[0 .. n) with lo <= x[i] <= hi, as [first, last] (last < first: none).  Two binary searches;
// each loop halves b - a
__device__ __forceinline__ void sg_axis_range(const float* __restrict__ x, int n, double lo, double hi, int& first, int& last) {
    int a = 0, b = n;
    while (a < b) {   // the first i with x[i] >= lo
        const int m = a + (b - a) / 2;
        if ((double)x[m] >= lo) b = m;
        else a = m + 1;
    }
    first = a;
    a = 0, b = n;
    while (a < b) {   // the first i with x[i] > hi
        const int m = a + (b - a) / 2;
        if ((double)x[m] > hi) b = m;
        else a = m + 1;
    }
    last = a - 1;
}

// One lane per triangle: validity, box, class.  info[1] |= 1 for a vertex that is not finite; such a triangle gets no box (the
// whole answer is NaN then)
__global__ __launch_bounds__(kSgThreads) void k_sg_setup(const float* __restrict__ tris, int n_faces, const float* __restrict__ xs,
                                                         int nx, const float* __restrict__ ys, int ny, const float* __restrict__ zs,
                                                         int nz, double trunc, int* __restrict__ rect, int* __restrict__ med,
                                                         int* __restrict__ huge, int* __restrict__ info) {
    const int f = blockIdx.x * kSgThreads + threadIdx.x;
    const unsigned lane = threadIdx.x & 63;
    int cls = -1;   // no class: beyond the end, not finite, or no node in the box.  Every lane reaches the ballots below
    if (f < n_faces) {
        const float* v = tris + (size_t)f * 9;
        int* rc = rect + 6 * (size_t)f;
        const float* axis[3] = {xs, ys, zs};
        const int len[3] = {nx, ny, nz};
        bool bad = false;
        double mn[3], mx[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double x0 = (double)v[c], x1 = (double)v[3 + c], x2 = (double)v[6 + c];
            bad = bad || !(fabs(x0) <= kMdFltMax) || !(fabs(x1) <= kMdFltMax) || !(fabs(x2) <= kMdFltMax);
            mn[c] = fmin(x0, fmin(x1, x2));
            mx[c] = fmax(x0, fmax(x1, x2));
        }
        if (bad) {
            atomicOr(&info[1], 1);
            for (int c = 0; c < 3; ++c) rc[2 * c] = 0, rc[2 * c + 1] = -1;
        } else {
            long long n = 1;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                // the closest point is a convex combination of the corners up to a few roundings, so a node farther than trunc from
                // the bounding box along this axis has d^2 > trunc^2; the slack is 2^-40 of the magnitudes involved, the rounding of
                // d^2 is below 2^-48 of them.  trunc = +inf: the whole axis
                const double slack = (fabs(mn[c]) + fabs(mx[c]) + (trunc < 1e300 ? trunc : 0.0)) * 0x1p-40;
                int first, last;
                sg_axis_range(axis[c], len[c], (mn[c] - trunc) - slack, (mx[c] + trunc) + slack, first, last);
                rc[2 * c] = first;
                rc[2 * c + 1] = last;
                n *= (long long)max(last - first + 1, 0);   // <= nx ny nz <= INT32_MAX
            }
            if (n > 0) cls = n <= kSgLaneNodes ? 0 : n <= kSgWaveNodes ? 1 : n <= kSgGroupNodes ? 2 : 3;
        }
    }
    // one atomicAdd per wave and class, not one per triangle: a hundred thousand increments of one counter take a millisecond
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const unsigned long long mask = __ballot(cls == c);
        if (!mask) continue;   // the same for all 64 lanes
        const int leader = __ffsll((long long)mask) - 1;
        int base = 0;
        if ((int)lane == leader) base = atomicAdd(&info[4 + c], __popcll(mask));   // the counters sum to at most n_faces
        base = __shfl(base, leader);
        const int slot = base + __popcll(mask & ((1ull << lane) - 1ull));
        if (cls == c && c == 2 && slot < n_faces) med[slot] = f;
        if (cls == c && c == 3 && slot < n_faces) huge[slot] = f;
    }
}

struct SgLattice {
    const float *xs, *ys, *zs;
    int ny, nz;
};

struct SgBox {   // a triangle's box as the walks take it: first node, h x d nodes per i-slab
    int i0, j0, k0, h, d;
};

// Nodes first, first + stride, ... < last of the box (i0, j0, k0) with h x d nodes per i-slab (k fastest, like the lattice itself)
// against triangle f.  PASS 0: the minimum of d^2.  PASS 1: the lowest id among the triangles that attain it.  Every node lies
// inside the lattice: i0 + row <= i1 < nx etc. by sg_axis_range.  Returns the tests made
template <int PASS>
__device__ __forceinline__ unsigned sg_walk(const float* __restrict__ tris, int f, const SgLattice& L, int i0, int j0, int k0, int h,
                                            int d, unsigned first, unsigned last, unsigned stride, double trunc2,
                                            unsigned long long* __restrict__ d2, int* __restrict__ face) {
#pragma clang fp contract(off)
    if (first >= last) return 0u;
    const float* v = tris + (size_t)f * 9;
    const D3 a = {(double)v[0], (double)v[1], (double)v[2]}, b = {(double)v[3], (double)v[4], (double)v[5]},
             c = {(double)v[6], (double)v[7], (double)v[8]};
    const unsigned hd = (unsigned)h * (unsigned)d;
    unsigned tests = 0u;
    // terminates: last - q strictly decreases (stride >= 1; q + stride <= 2^31 + 2^16 does not wrap)
    for (unsigned q = first; q < last; q += stride) {
        const unsigned ri = q / hd, rem = q - ri * hd, rj = rem / (unsigned)d, rk = rem - rj * (unsigned)d;
        const int i = i0 + (int)ri, j = j0 + (int)rj, k = k0 + (int)rk;
        const D3 p = {(double)L.xs[i], (double)L.ys[j], (double)L.zs[k]};
        double wa, wb, wc;
        closest_on_triangle(p, a, b, c, wa, wb, wc);
        const D3 cp = {wa * a.x + wb * b.x + wc * c.x, wa * a.y + wb * b.y + wc * c.y, wa * a.z + wb * b.z + wc * c.z};
        const D3 dv = dsub(p, cp);
        const double dd = ddot(dv, dv);
        ++tests;
        if (!(dd <= trunc2)) continue;   // a NaN is never a distance
        const size_t node = ((size_t)i * (size_t)L.ny + (size_t)j) * (size_t)L.nz + (size_t)k;
        const unsigned long long bits = (unsigned long long)__double_as_longlong(dd);   // dd >= +0: ordered like the double
        if (PASS == 0) {
            if (bits < d2[node]) atomicMin(&d2[node], bits);
        } else {
            if (bits == d2[node] && f < face[node]) atomicMin(&face[node], f);
        }
    }
    return tests;
}

// the tests of a wave -> one 64-bit atomicAdd (PASS 0 only).  Called by all 64 lanes
__device__ __forceinline__ void sg_count(unsigned long long tests, int* __restrict__ info) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) tests += __shfl_xor(tests, o);
    if ((threadIdx.x & 63) == 0 && tests) atomicAdd(reinterpret_cast<unsigned long long*>(info + 2), tests);
}

// lane and wave classes
template <int PASS>
__global__ __launch_bounds__(kSgThreads) void k_sg_walk(const float* __restrict__ tris, const int* __restrict__ rect, int n_faces,
                                                        SgLattice L, double trunc2, unsigned long long* __restrict__ d2,
                                                        int* __restrict__ face, int* __restrict__ info) {
    const unsigned lane = threadIdx.x & 63;
    const long long wave = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((long long)gridDim.x * blockDim.x) >> 6;
    unsigned long long tests = 0ull;
    if (info[1] == 0) {
        // A wave holds kSgWaveFaces consecutive faces, one in each of its first lanes: the wave class takes the whole wave for one
        // face after the other, and fewer faces a wave are more waves in flight.  terminates: n_faces - base strictly decreases;
        // base is the same for all 64 lanes, so they reach the ballot together; lanes without a face carry n = 0
        for (long long base = wave * kSgWaveFaces; base < n_faces; base += n_waves * kSgWaveFaces) {
            const long long f = base + lane;
            int i0 = 0, j0 = 0, k0 = 0, h = 1, d = 1;
            long long n = 0;
            if (lane < (unsigned)kSgWaveFaces && f < n_faces) {
                const int* rc = rect + 6 * (size_t)f;
                i0 = rc[0], j0 = rc[2], k0 = rc[4], h = rc[3] - rc[2] + 1, d = rc[5] - rc[4] + 1;
                const int w = rc[1] - rc[0] + 1;
                if (w < 1 || h < 1 || d < 1) h = 1, d = 1;
                else n = (long long)w * h * d;
            }
            if (n > 0 && n <= kSgLaneNodes) tests += sg_walk<PASS>(tris, (int)f, L, i0, j0, k0, h, d, 0u, (unsigned)n, 1u, trunc2, d2, face);
            mesh_wave_turns(n > kSgLaneNodes && n <= kSgWaveNodes, [&](int src) {
                const int bi0 = __shfl(i0, src), bj0 = __shfl(j0, src), bk0 = __shfl(k0, src), bh = __shfl(h, src), bd = __shfl(d, src);
                const unsigned bn = (unsigned)__shfl((int)n, src);
                tests += sg_walk<PASS>(tris, (int)(base + src), L, bi0, bj0, bk0, bh, bd, lane, bn, 64u, trunc2, d2, face);
            });
        }
    }
    if (PASS == 0) sg_count(tests, info);
}

// workgroup and many-workgroup classes
template <int PASS>
__global__ __launch_bounds__(kSgThreads) void k_sg_walk_lists(const float* __restrict__ tris, const int* __restrict__ rect,
                                                              const int* __restrict__ med, const int* __restrict__ huge, int n_faces,
                                                              SgLattice L, double trunc2, unsigned long long* __restrict__ d2,
                                                              int* __restrict__ face, int* __restrict__ info) {
    unsigned long long tests = 0ull;
    if (info[1] == 0) {
        mesh_list_walk<kSgParts, kSgThreads, SgBox>(
            med, (unsigned)min(max(info[6], 0), n_faces), huge, (unsigned)min(max(info[7], 0), n_faces),
            [&](int f, SgBox& b) {
                if ((unsigned)f >= (unsigned)n_faces) return 0u;
                const int* rc = rect + 6 * (size_t)f;
                const int w = rc[1] - rc[0] + 1, h = rc[3] - rc[2] + 1, d = rc[5] - rc[4] + 1;
                if (w < 1 || h < 1 || d < 1) return 0u;
                b.i0 = rc[0], b.j0 = rc[2], b.k0 = rc[4], b.h = h, b.d = d;
                return (unsigned)((long long)w * h * d);   // <= nx ny nz <= INT32_MAX
            },
            [&](int f, const SgBox& b, unsigned first, unsigned last, unsigned stride) {
                tests += sg_walk<PASS>(tris, f, L, b.i0, b.j0, b.k0, b.h, b.d, first, last, stride, trunc2, d2, face);
            });
    }
    if (PASS == 0) sg_count(tests, info);
}

// the signed value of meshing.signed_distance: (inside ? -1 : +1) * min(sqrt(d2), trunc) in float64 (a NaN stays one), rounded once
__device__ __forceinline__ float sg_signed(double d2, bool inside, double trunc) {
    const double r = sqrt(d2);
    const double m = (r != r) ? r : (r < trunc ? r : trunc);
    return (float)(inside ? -m : m);
}

__global__ __launch_bounds__(kSgThreads) void k_sg_finish(SgLattice L, long long n, double trunc, double trunc2,
                                                          const uint8_t* __restrict__ occ, double* __restrict__ d2, int* __restrict__ face,
                                                          float* __restrict__ sdf, int* __restrict__ info) {
    __shared__ unsigned s_band[kSgThreads / 64];
    const long long step = (long long)gridDim.x * blockDim.x;
    const long long plane = (long long)L.ny * L.nz;
    const bool bad_mesh = info[1] != 0;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    unsigned band = 0u;
    // terminates: n - p strictly decreases
    for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += step) {
        const long long i = p / plane, r = p - i * plane, j = r / L.nz, k = r - j * L.nz;
        const double x = (double)L.xs[i], y = (double)L.ys[j], z = (double)L.zs[k];
        double v = d2[p];   // the minimum, or +inf: no triangle was within trunc (with trunc = +inf: there is no triangle)
        if (bad_mesh || !(fabs(x) <= kMdFltMax) || !(fabs(y) <= kMdFltMax) || !(fabs(z) <= kMdFltMax)) v = nan;
        const bool in_band = v <= trunc2 && v < __longlong_as_double((long long)kSgInfBits);
        d2[p] = v;
        if (face) face[p] = in_band ? face[p] : -1;
        if (sdf) sdf[p] = sg_signed(v, occ && occ[p] != 0, trunc);
        band += in_band ? 1u : 0u;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) band += __shfl_xor(band, o);
    if ((threadIdx.x & 63) == 0) s_band[threadIdx.x >> 6] = band;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned t = 0u;
        for (int w = 0; w < kSgThreads / 64; ++w) t += s_band[w];
        if (t) atomicAdd(&info[0], (int)t);   // <= n <= INT32_MAX in all
    }
}

}  // namespace
