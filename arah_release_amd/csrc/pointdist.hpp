// pointdist.hpp -- exact nearest point of a LARGE cloud (a scan: 1e5 .. 1e7 points on a sheet) for every query point, and the
// per-side reduction of the geometry scores over meshes AND clouds (DESIGN.md "Scoring against point clouds").  The structure
// is meshdist.hpp's with points in place of triangles: a point lies in exactly one cell, so there is no span and no big list.
//
//   k_pd_stats     per workgroup: bounding box of the FINITE points and their number
//   k_pd_coarse    one workgroup folds them: the box, the coarse lattice (kPdCoarse cubic cells along the longest axis)
//   k_pd_mark      per point: its coarse cell is occupied (every writer stores the same 1)
//   k_pd_header    one workgroup counts the occupied coarse cells and the occupied 2x2x2 blocks of them, and sizes the cells
//                  from the two counts (below) under the cell budget -> PdHeader
//   k_pd_bin<0>    per finite point: one count for its cell
//   k_md_scan      exclusive scan of the counts (meshdist.hpp's, on this header)
//   k_pd_bin<1>    the same walk again: the point goes to a slot of its cell (slot by integer atomic: the order inside a cell is
//                  free) as x, y, z and its index in one 16-byte record, so a query reads a cell as one contiguous run
//   k_md_dt<A>     Chebyshev distance transform of the occupied cells (meshdist.hpp's)
//   k_pd_nearest   one thread per query: rings of cells around the cell of the query's clamp onto the box, starting at the first
//                  non-empty ring
//
// Cell size.  The workload is a 2-D sheet in a 3-D box: box volume / n says nothing about how many points share a cell.  What
// is measured instead: M, the occupied cells of a coarse lattice of side g, and M2, the occupied 2x2x2 blocks of it.  Their ratio
// is the cloud's box-counting dimension at that scale, dim = log2(M / M2) clamped to [1, 3], and the occupied cells at side h are
// estimated as M (g / h)^dim.  h is chosen so that this estimate equals n / kPdTarget -- kPdTarget points per OCCUPIED cell --
// and then grown until the lattice fits the cell budget (8 cells per point, at most 2^24) and kPdMaxSide cells per axis.  A cloud
// too sparse for the coarse lattice (fewer than kPdTarget points per coarse cell) gets cells coarser than g by the volume rule.
// Floors: h >= 2^-30 of the coordinates' magnitude (the slack of the bounds stays far below a cell) and h = 1 for a cloud of
// zero extent; an axis of zero extent has one cell.  The choice changes the cost of a query, never its result.
//
// Everything is sized by n alone (one record per point, the cell budget, the fixed coarse lattice): no capacity to overflow,
// nothing truncated, no host synchronisation.  Non-finite points are skipped by every pass and counted in the header (n_bad).
//
// Exactness: meshdist.hpp's argument.  pd_cell_of() is monotone, so a point lies within its cell's bounds up to the slack.  A
// query ends when a float64 LOWER bound (with slack) on the distance to everything outside the finished rings is STRICTLY greater
// than its best d^2, so every tie is examined and the result is the lexicographic minimum of (d^2, index): the order of the
// records cannot change it.  A query outside the box is bounded through its clamp.  Rings are clipped to what the best d^2 can
// reach.  Every loop runs over cells of the lattice or records of a cell: bounded whatever the input.  Included by arah_hip.hip
// after meshdist.hpp.
#pragma once

namespace {

constexpr int kPdThreads = 256;
constexpr int kPdQueryThreads = 64;
constexpr int kPdStatBlocks = 256;
constexpr int kPdCoarse = 64;                                       // coarse cells along the longest axis
constexpr int kPdCoarseSide = kPdCoarse + 1;                        // ... the point at hi may open one more
constexpr int kPdCoarseCap = kPdCoarseSide * kPdCoarseSide * kPdCoarseSide;
constexpr int kPdMaxSide = 1024;                                    // most cells along one axis
constexpr int kPdMinCells = 4096, kPdMaxCells = 1 << 24;
constexpr double kPdTarget = 4.0;                                   // points per occupied cell aimed at
constexpr int kPdMaxThresholds = 16;
constexpr size_t kPdHeaderBytes = 256;

struct PdHeader {
    double lo[3], hi[3];   // bounding box of the finite points
    double h, inv_h;       // cell side
    double g, inv_g;       // coarse cell side
    double dim;            // measured box-counting dimension, clamped to [1, 3]
    int n[3];              // cells per axis
    int n_cells, n_refs;   // n_refs: the finite points (records)
    int n_bad;             // points with a non-finite coordinate: skipped
    int cn[3];             // coarse cells per axis
    int c_occ, c_occ2;     // occupied coarse cells, occupied 2x2x2 blocks of them
};
static_assert(sizeof(PdHeader) <= kPdHeaderBytes, "header");

struct PdRecord {
    float x, y, z;
    int index;
};
static_assert(sizeof(PdRecord) == 16, "record");

struct PdIndex {
    PdHeader* hdr;
    double* stat;          // [kPdStatBlocks][8]: lo xyz, hi xyz, finite points, unused
    int* coarse;           // [kPdCoarseCap] occupancy of the coarse lattice
    int* cell_base;        // [cap_cells + 1]
    int* cell_count;       // [cap_cells]
    uint8_t* dt[2];        // [cap_cells] each
    PdRecord* recs;        // [n]
    int cap_cells;
    size_t bytes;
};

inline int pd_cap_cells(long long n) {
    long long c = 8 * n;
    return (int)(c < kPdMinCells ? kPdMinCells : c > kPdMaxCells ? kPdMaxCells : c);
}

__device__ __forceinline__ bool pd_finite(double x, double y, double z) {
    return fabs(x) <= kMdFltMax && fabs(y) <= kMdFltMax && fabs(z) <= kMdFltMax;   // inf and NaN fail
}

// cell of coordinate x along axis a: monotone in x, clamped into the grid
__device__ __forceinline__ int pd_cell_of(const PdHeader& H, int a, double x) {
    const double u = floor((x - H.lo[a]) * H.inv_h);
    const int top = H.n[a] - 1;
    return u <= 0.0 ? 0 : (u >= (double)top ? top : (int)u);
}

__device__ __forceinline__ int pd_coarse_of(const PdHeader& H, int a, double x) {
    const double u = floor((x - H.lo[a]) * H.inv_g);
    const int top = H.cn[a] - 1;
    return u <= 0.0 ? 0 : (u >= (double)top ? top : (int)u);
}

__global__ __launch_bounds__(kPdThreads) void k_pd_stats(const float* __restrict__ pts, int n, double* __restrict__ stat) {
    __shared__ double red[7][kPdThreads];
    const int t = threadIdx.x;
    double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300}, cnt = 0.0;
    for (int i = blockIdx.x * kPdThreads + t; i < n; i += kPdStatBlocks * kPdThreads) {
        const double x[3] = {(double)pts[(size_t)i * 3], (double)pts[(size_t)i * 3 + 1], (double)pts[(size_t)i * 3 + 2]};
        if (!pd_finite(x[0], x[1], x[2])) continue;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            lo[c] = fmin(lo[c], x[c]);
            hi[c] = fmax(hi[c], x[c]);
        }
        cnt += 1.0;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        red[c][t] = lo[c];
        red[3 + c][t] = hi[c];
    }
    red[6][t] = cnt;
    __syncthreads();
    for (int s = kPdThreads / 2; s > 0; s >>= 1) {
        if (t < s) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                red[c][t] = fmin(red[c][t], red[c][t + s]);
                red[3 + c][t] = fmax(red[3 + c][t], red[3 + c][t + s]);
            }
            red[6][t] += red[6][t + s];   // whole numbers below 2^53: exact in any order
        }
        __syncthreads();
    }
    if (t < 7) stat[(size_t)blockIdx.x * 8 + t] = red[t][0];
}

// the box and the coarse lattice; the rest of the header is k_pd_header's
__global__ __launch_bounds__(kPdStatBlocks) void k_pd_coarse(const double* __restrict__ stat, int n, PdHeader* __restrict__ hdr) {
    __shared__ double red[7][kPdStatBlocks];
    const int t = threadIdx.x;
#pragma unroll
    for (int c = 0; c < 7; ++c) red[c][t] = stat[(size_t)t * 8 + c];
    __syncthreads();
    for (int s = kPdStatBlocks / 2; s > 0; s >>= 1) {
        if (t < s) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                red[c][t] = fmin(red[c][t], red[c][t + s]);
                red[3 + c][t] = fmax(red[3 + c][t], red[3 + c][t + s]);
            }
            red[6][t] += red[6][t + s];
        }
        __syncthreads();
    }
    if (t != 0) return;
    PdHeader H;
    const int n_finite = (int)red[6][0];
    double side = 0.0;
    for (int c = 0; c < 3; ++c) {
        H.lo[c] = n_finite > 0 ? red[c][0] : 0.0;
        H.hi[c] = n_finite > 0 ? red[3 + c][0] : 0.0;
        side = fmax(side, H.hi[c] - H.lo[c]);
    }
    double g = side / (double)kPdCoarse;
    if (!(g > 0.0)) g = 1.0;                                         // every finite point is the same point, or there is none
    H.g = g;
    H.inv_g = 1.0 / g;
    for (int c = 0; c < 3; ++c) H.cn[c] = (int)fmin(floor((H.hi[c] - H.lo[c]) / g) + 1.0, (double)kPdCoarseSide);
    H.h = g;
    H.inv_h = H.inv_g;
    H.dim = 0.0;
    H.n[0] = H.n[1] = H.n[2] = 1;
    H.n_cells = 1;
    H.n_refs = n_finite;
    H.n_bad = n - n_finite;
    H.c_occ = H.c_occ2 = 0;
    *hdr = H;
}

__global__ __launch_bounds__(kPdThreads) void k_pd_mark(const float* __restrict__ pts, int n, const PdHeader* __restrict__ hdr,
                                                        int* __restrict__ coarse) {
    const int i = blockIdx.x * kPdThreads + threadIdx.x;
    if (i >= n) return;
    const PdHeader H = *hdr;
    const double x = (double)pts[(size_t)i * 3], y = (double)pts[(size_t)i * 3 + 1], z = (double)pts[(size_t)i * 3 + 2];
    if (!pd_finite(x, y, z)) return;
    const int cx = pd_coarse_of(H, 0, x), cy = pd_coarse_of(H, 1, y), cz = pd_coarse_of(H, 2, z);
    coarse[(cz * H.cn[1] + cy) * H.cn[0] + cx] = 1;                  // < cn0 cn1 cn2 <= kPdCoarseCap; every writer stores 1
}

__global__ __launch_bounds__(1024) void k_pd_header(const int* __restrict__ coarse, int cap_cells, PdHeader* __restrict__ hdr) {
    __shared__ int occ[2];
    const int t = threadIdx.x;
    if (t < 2) occ[t] = 0;
    __syncthreads();
    const int cx = hdr->cn[0], cy = hdr->cn[1], cz = hdr->cn[2];
    const int px = (cx + 1) / 2, py = (cy + 1) / 2, pz = (cz + 1) / 2;
    int m1 = 0, m2 = 0;
    for (int b = t; b < px * py * pz; b += 1024) {                   // one 2x2x2 block of coarse cells per trip
        const int bx = b % px, by = (b / px) % py, bz = b / (px * py);
        int inside = 0;
        for (int k = 0; k < 8; ++k) {
            const int x = 2 * bx + (k & 1), y = 2 * by + ((k >> 1) & 1), z = 2 * bz + (k >> 2);
            if (x < cx && y < cy && z < cz) inside += coarse[(z * cy + y) * cx + x] != 0;
        }
        m1 += inside;
        m2 += inside > 0;
    }
    atomicAdd(&occ[0], m1);                                          // integer sums: the order is free
    atomicAdd(&occ[1], m2);
    __syncthreads();
    if (t != 0) return;
    PdHeader H = *hdr;
    H.c_occ = occ[0];
    H.c_occ2 = occ[1];
    double side = 0.0, mag = 0.0;
    for (int c = 0; c < 3; ++c) {
        side = fmax(side, H.hi[c] - H.lo[c]);
        mag = fmax(mag, fmax(fabs(H.lo[c]), fabs(H.hi[c])));
    }
    double h = H.g;
    H.dim = 1.0;
    if (H.c_occ > 0 && H.n_refs > 0) {
        H.dim = fmin(3.0, fmax(1.0, log2((double)H.c_occ / (double)H.c_occ2)));
        const double ratio = ((double)H.n_refs / kPdTarget) / (double)H.c_occ;   // occupied cells wanted per occupied coarse cell
        h = ratio >= 1.0 ? H.g / pow(ratio, 1.0 / H.dim) : H.g * cbrt(1.0 / ratio);
    }
    if (!(side > 0.0) || !(h > 0.0)) h = 1.0;                        // zero extent: one cell
    h = fmax(h, side / (double)(kPdMaxSide - 1));
    h = fmax(h, mag * 0x1p-30);
    bool fits = false;
    for (int it = 0; it < 256 && !fits; ++it) {                      // the cell budget: grow h until the grid fits
        double cells = 1.0;
        bool clamped = false;
        for (int c = 0; c < 3; ++c) {
            const double n = floor((H.hi[c] - H.lo[c]) / h) + 1.0;
            clamped = clamped || n > (double)kPdMaxSide;
            H.n[c] = (int)fmin(n, (double)kPdMaxSide);
            cells *= (double)H.n[c];
        }
        if (cells <= (double)cap_cells && !clamped) {
            fits = true;
            break;
        }
        h *= 1.25;
    }
    if (!fits) {                                                     // not reached for finite boxes; one cell is always right
        h = 2.0 * side + 1.0;
        H.n[0] = H.n[1] = H.n[2] = 1;
    }
    H.h = h;
    H.inv_h = 1.0 / h;
    H.n_cells = H.n[0] * H.n[1] * H.n[2];
    H.n_refs = 0;                                                    // k_md_scan writes the total
    *hdr = H;
}

// FILL false: counts per cell;  true: the records (cell_count counts DOWN to hand out the slots)
template <bool FILL>
__global__ __launch_bounds__(kPdThreads) void k_pd_bin(const float* __restrict__ pts, int n, const PdHeader* __restrict__ hdr,
                                                       int* __restrict__ cell_count, const int* __restrict__ cell_base,
                                                       PdRecord* __restrict__ recs) {
    const int i = blockIdx.x * kPdThreads + threadIdx.x;
    if (i >= n) return;
    const PdHeader H = *hdr;
    const float fx = pts[(size_t)i * 3], fy = pts[(size_t)i * 3 + 1], fz = pts[(size_t)i * 3 + 2];
    if (!pd_finite((double)fx, (double)fy, (double)fz)) return;
    const int cell = (pd_cell_of(H, 2, (double)fz) * H.n[1] + pd_cell_of(H, 1, (double)fy)) * H.n[0] + pd_cell_of(H, 0, (double)fx);
    if (FILL) {
        const int slot = atomicSub(&cell_count[cell], 1) - 1;        // >= 0: the count pass counted this point
        recs[cell_base[cell] + slot] = PdRecord{fx, fy, fz, i};      // < n_refs <= n
    } else {
        atomicAdd(&cell_count[cell], 1);                             // cell < n_cells <= cap_cells
    }
}

// queries [Q][3] float32 -> d2 [Q] f64, nearest [Q] i32, tested [Q] (or null): the point tests the query made
__global__ __launch_bounds__(kPdQueryThreads) void k_pd_nearest(const PdHeader* __restrict__ hdr, const int* __restrict__ cell_base,
                                                                const uint8_t* __restrict__ dt, const PdRecord* __restrict__ recs,
                                                                const float* __restrict__ qs, int n_q, double* __restrict__ d2_out,
                                                                int* __restrict__ nearest_out, int* __restrict__ tested_out) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_q) return;
    const PdHeader H = *hdr;
    const double pa[3] = {(double)qs[(size_t)i * 3], (double)qs[(size_t)i * 3 + 1], (double)qs[(size_t)i * 3 + 2]};
    if (!pd_finite(pa[0], pa[1], pa[2])) {
        d2_out[i] = __longlong_as_double(0x7ff8000000000000ll);
        nearest_out[i] = -1;
        if (tested_out) tested_out[i] = 0;
        return;
    }
    double best = 1e300;   // above every d^2 of finite float32 coordinates (< 2e78)
    int bidx = -1, tested = 0;
    if (H.n_refs > 0) {
        // the clamp onto the box, its cell, and what the clamp gives away
        double pc[3], slack[3], off2 = 0.0;
        int cp[3], rmax = 0;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            pc[a] = fmin(fmax(pa[a], H.lo[a]), H.hi[a]);
            const double o = pa[a] - pc[a];
            off2 += o * o;
            cp[a] = pd_cell_of(H, a, pc[a]);
            rmax = max(rmax, max(cp[a], H.n[a] - 1 - cp[a]));
            // absolute slack of every bound along this axis: 2^-20 cells (cell_of rounds within 2^-40 of a cell) and 2^-45 of
            // the coordinates' magnitude (the bounds' own subtractions round within 2^-52 of it)
            slack[a] = H.h * 0x1p-20 + (fabs(H.lo[a]) + fabs(H.hi[a]) + fabs(pa[a])) * 0x1p-45;
        }
        const double keep = 1.0 - 0x1p-30;   // ... and of squaring and adding them
        // lower bound of |p - t| along axis a for every point t of cell index c
        auto axis_gap = [&](int a, int c) -> double {
            const double below = (H.lo[a] + (double)c * H.h) - slack[a] - pa[a];
            const double above = pa[a] - (H.lo[a] + (double)(c + 1) * H.h) - slack[a];
            return fmax(0.0, fmax(below, above));
        };
        // first / last cell along axis a that reaches into [p - reach, p + reach]; an empty range when none does
        auto reach_lo = [&](int a, double reach) -> int {
            const double u = floor((pa[a] - reach - H.lo[a]) * H.inv_h) - 1.0;
            return u <= 0.0 ? 0 : (u >= (double)H.n[a] ? H.n[a] : (int)u);
        };
        auto reach_hi = [&](int a, double reach) -> int {
            const double u = floor((pa[a] + reach - H.lo[a]) * H.inv_h) + 1.0;
            return u < 0.0 ? -1 : (u >= (double)(H.n[a] - 1) ? H.n[a] - 1 : (int)u);
        };
        const int nx = H.n[0], ny = H.n[1], nz = H.n[2];
        for (int r = (int)dt[(cp[2] * ny + cp[1]) * nx + cp[0]]; r <= rmax; ++r) {
            int z0 = max(cp[2] - r, 0), z1 = min(cp[2] + r, nz - 1);
            int y0 = max(cp[1] - r, 0), y1 = min(cp[1] + r, ny - 1);
            int x0 = max(cp[0] - r, 0), x1 = min(cp[0] + r, nx - 1);
            if (best < 1e290) {
                // only the slab of cells within sqrt(best) of the query can pass the gap tests below: the ring is clipped to
                // it, widened by 2^-20 of the reach (its rounding and the bounds') and by one cell on either side (the slack)
                const double reach = sqrt(best) * (1.0 + 0x1p-20) + H.h;
                z0 = max(z0, reach_lo(2, reach)), z1 = min(z1, reach_hi(2, reach));
                y0 = max(y0, reach_lo(1, reach)), y1 = min(y1, reach_hi(1, reach));
                x0 = max(x0, reach_lo(0, reach)), x1 = min(x1, reach_hi(0, reach));
            }
            for (int z = z0; z <= z1; ++z) {
                const double gz = axis_gap(2, z), gz2 = gz * gz;
                if (gz2 * keep > best) continue;
                const bool on_z = z == cp[2] - r || z == cp[2] + r;
                for (int y = y0; y <= y1; ++y) {
                    const double gy = axis_gap(1, y), gzy2 = gz2 + gy * gy;
                    if (gzy2 * keep > best) continue;
                    const bool shell = on_z || y == cp[1] - r || y == cp[1] + r;
                    // a row of the ring's shell is walked whole; an inner row contributes its two ends
                    const int step = shell ? 1 : max(2 * r, 1);
                    for (int x = shell ? x0 : cp[0] - r; x <= x1; x += step) {
                        if (x < x0) continue;
                        const double gx = axis_gap(0, x);
                        if ((gzy2 + gx * gx) * keep > best) continue;
                        const int cell = (z * ny + y) * nx + x;
                        const int e0 = cell_base[cell], e1 = cell_base[cell + 1];
                        for (int k = e0; k < e1; ++k) {
                            const PdRecord q = recs[k];
                            const double dx = pa[0] - (double)q.x, dy = pa[1] - (double)q.y, dz = pa[2] - (double)q.z;
                            const double d2 = (dx * dx + dy * dy) + dz * dz;
                            if (d2 < best || (d2 == best && q.index < bidx)) {
                                best = d2;
                                bidx = q.index;
                            }
                            ++tested;
                        }
                    }
                }
            }
            // everything not examined yet lies outside the block of cells [cp - r, cp + r] along some axis
            double m = 1e300;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                if (cp[a] - r > 0) m = fmin(m, pc[a] - (H.lo[a] + (double)(cp[a] - r) * H.h) - slack[a]);
                if (cp[a] + r + 1 < H.n[a]) m = fmin(m, (H.lo[a] + (double)(cp[a] + r + 1) * H.h) - pc[a] - slack[a]);
            }
            if (m == 1e300) break;   // the block is the grid
            m = fmax(m, 0.0);
            if ((m * m + off2) * keep > best) break;
        }
    }
    d2_out[i] = bidx >= 0 ? best : __longlong_as_double(0x7ff0000000000000ll);   // no finite point: +inf
    nearest_out[i] = bidx;
    if (tested_out) tested_out[i] = tested;
}

// ---- the per-side scores ---------------------------------------------------------------------------------------------------
struct PdSide {
    const double* d2;         // [n]
    const double* n_sample;   // [n][3] unit normals of the samples, or null
    const double* n_other;    // [n_other][3] unit normals of the other side's elements, or null
    const int* idx;           // [n] element of the other side each sample was matched to (with n_other)
    const double* thr2;       // [n_thr] squared thresholds
    int n, n_other_count, n_thr;
};

// workgroup b: samples [256 b, 256 b + 256) -> part[b][4] = sum d, sum d^2, sum c, max d (fixed tree), cnt[b][16] = samples
// with d2 <= thr2[t]
__global__ __launch_bounds__(kPdThreads) void k_pd_scores_part(PdSide s, double* __restrict__ part, int* __restrict__ cnt) {
#pragma clang fp contract(off)
    __shared__ double red[4][kPdThreads];
    __shared__ int within[kPdMaxThresholds];
    const int t = threadIdx.x;
    if (t < kPdMaxThresholds) within[t] = 0;
    __syncthreads();
    const int k = (int)blockIdx.x * kPdThreads + t;
    double d = 0.0, d2 = 0.0, c = 0.0;
    if (k < s.n) {
        d2 = s.d2[k];
        d = sqrt(d2);
        if (s.n_sample && s.n_other) {
            const int g = s.idx[k];
            if (g >= 0 && g < s.n_other_count) {
                const double* a = s.n_sample + (size_t)k * 3;
                const double* b = s.n_other + (size_t)g * 3;
                c = fabs((a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]);
            } else {
                c = __longlong_as_double(0x7ff8000000000000ll);
            }
        }
        for (int q = 0; q < s.n_thr; ++q)
            if (d2 <= s.thr2[q]) atomicAdd(&within[q], 1);           // integer, in LDS: the order is free
    }
    red[0][t] = d;
    red[1][t] = d2;
    red[2][t] = c;
    red[3][t] = d;
    __syncthreads();
    for (int w = kPdThreads / 2; w > 0; w >>= 1) {
        if (t < w) {
            red[0][t] += red[0][t + w];
            red[1][t] += red[1][t + w];
            red[2][t] += red[2][t + w];
            // a NaN distance must not vanish in fmax
            const double u = red[3][t], v = red[3][t + w];
            red[3][t] = (u != u || v != v) ? u + v : fmax(u, v);
        }
        __syncthreads();
    }
    if (t < 4) part[(size_t)blockIdx.x * 4 + t] = red[t][0];
    if (t < kPdMaxThresholds) cnt[(size_t)blockIdx.x * kPdMaxThresholds + t] = within[t];
}

// one workgroup: the partials in index order (thread t takes t, t + 256, ...; then the fixed tree) -> sums[6] = sum d, sum d^2,
// sum c, max d, samples in the distance sums, samples in the normal sum;  within[n_thr] int64
__global__ __launch_bounds__(kPdThreads) void k_pd_scores_finish(const double* __restrict__ part, const int* __restrict__ cnt, int blocks,
                                                                 int n, int has_normals, int n_thr, double* __restrict__ sums,
                                                                 long long* __restrict__ within) {
#pragma clang fp contract(off)
    __shared__ double red[4][kPdThreads];
    __shared__ long long ired[kPdThreads];
    const int t = threadIdx.x;
    double a[4] = {0.0, 0.0, 0.0, 0.0};
    for (int k = t; k < blocks; k += kPdThreads) {
        a[0] += part[(size_t)k * 4];
        a[1] += part[(size_t)k * 4 + 1];
        a[2] += part[(size_t)k * 4 + 2];
        const double v = part[(size_t)k * 4 + 3];
        a[3] = (a[3] != a[3] || v != v) ? a[3] + v : fmax(a[3], v);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) red[q][t] = a[q];
    __syncthreads();
    for (int w = kPdThreads / 2; w > 0; w >>= 1) {
        if (t < w) {
            red[0][t] += red[0][t + w];
            red[1][t] += red[1][t + w];
            red[2][t] += red[2][t + w];
            const double u = red[3][t], v = red[3][t + w];
            red[3][t] = (u != u || v != v) ? u + v : fmax(u, v);
        }
        __syncthreads();
    }
    if (t < 4) sums[t] = red[t][0];
    if (t == 4) sums[4] = (double)n;
    if (t == 5) sums[5] = has_normals ? (double)n : 0.0;
    for (int q = 0; q < n_thr; ++q) {                                // n_thr is uniform: every thread makes every trip
        long long v = 0;
        for (int k = t; k < blocks; k += kPdThreads) v += (long long)cnt[(size_t)k * kPdMaxThresholds + q];
        __syncthreads();
        ired[t] = v;
        __syncthreads();
        for (int w = kPdThreads / 2; w > 0; w >>= 1) {
            if (t < w) ired[t] += ired[t + w];
            __syncthreads();
        }
        if (t == 0) within[q] = ired[0];
    }
}

}  // namespace
