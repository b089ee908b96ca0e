// meshdist.hpp -- exact point-to-mesh distance against LARGE triangle soups (a 256^3 marching-cubes mesh: a few 1e5
// triangles), for the geometry scores of DESIGN.md "Geometry metrics on the device".  meshquery.hpp walks every triangle for
// every point; this is the same per-triangle arithmetic (closest_on_triangle and the closest-point / d^2 lines of
// k_mesh_query, float64 on the float32 vertices and points) behind a uniform grid of triangle references:
//
//   k_md_stats    per workgroup: bounding box of the vertices, sum of the triangles' largest box extents
//   k_md_header   one workgroup folds them: cell size h = 2 x the mean extent, grid dimensions, MdHeader
//   k_md_bin<0>   per triangle: the cells its box overlaps; at most kMdSpan of them -> one count per cell, more -> the
//                 triangle goes to the `big` list that every query walks first
//   k_md_scan     exclusive scan of the cell counts (one workgroup, the length on the device)
//   k_md_bin<1>   the same walk again: a reference per overlapped cell (slot by atomic: the order inside a cell is free)
//   k_md_dt<A>    Chebyshev distance transform of the occupied cells, one axis after the other (uint8, 255 = ">= 255")
//   k_md_closest  one thread per query point: big list, then rings of cells around the cell of the point's clamp onto
//                 the box, starting at the first non-empty ring
//
// The size of everything is fixed by the triangle count (kMdSpan references per triangle at most, one big-list slot per
// triangle, a cell budget): there is no capacity to overflow and nothing is ever truncated.
//
// Exactness.  cell_of() is monotone in the coordinate, so every point of a triangle lies in a cell that references the
// triangle (or the triangle is in the big list).  A query ends when a LOWER bound on the distance to everything outside the
// rings it has finished is STRICTLY greater than its best d^2, so every tie is examined, and the result is the lexicographic
// minimum of (d^2, face index): the order of the references cannot change it.  The bounds are float64 with an absolute slack
// (`slack` in k_md_closest) that covers the rounding of cell_of() and of the bounds themselves.  A query point outside the box is bounded
// through its clamp onto the box: every triangle lies in the box, so along each axis the clamp is at least as near to it as
// the point, and the squared offset point -> clamp adds to the bound.  Every ring is clipped to the slab of cells within
// sqrt(best d^2) of the point before it is walked, and a row or a cell that the point's own distance to it rules out is
// skipped: a query far outside the box walks the cells it can reach, not the lattice.  The clip needs a best d^2: a query whose
// big list was empty walks its first non-empty ring unclipped -- one shell, O(r^2) gap tests -- and is clipped from the next ring
// on.  The termination bound does not depend on the clip.  Included by arah_hip.hip after meshquery.hpp.
#pragma once

namespace {

constexpr int kMdThreads = 256;
constexpr int kMdQueryThreads = 64;
constexpr int kMdStatBlocks = 256;
constexpr int kMdSpan = 8;                 // most cells a triangle is referenced from
constexpr int kMdMaxSide = 1024;           // most cells along one axis
constexpr int kMdMinCells = 4096, kMdMaxCells = 1 << 22;
constexpr size_t kMdHeaderBytes = 256;
constexpr double kMdFltMax = 3.4028234663852886e38;   // the largest finite float32: inf and NaN fail |x| <= it

struct MdHeader {
    double lo[3], hi[3];   // bounding box of the vertices
    double h, inv_h;       // cell side
    int n[3];              // cells per axis
    int n_cells, n_refs, n_big;
    int status;            // 0, or 1: a vertex is not finite (queries answer NaN / -1)
};
static_assert(sizeof(MdHeader) <= kMdHeaderBytes, "header");

struct MdIndex {
    MdHeader* hdr;
    double* stat;          // [kMdStatBlocks][8]: lo xyz, hi xyz, sum of extents, unused
    int* cell_base;        // [cap_cells + 1]
    int* cell_count;       // [cap_cells]
    uint8_t* dt[2];        // [cap_cells] each
    int* refs;             // [kMdSpan * F]
    int* big;              // [F]
    int cap_cells;
    size_t bytes;
};

inline int md_cap_cells(long long F) {
    long long c = 4 * F;
    return (int)(c < kMdMinCells ? kMdMinCells : c > kMdMaxCells ? kMdMaxCells : c);
}

// cell of coordinate x along axis a: monotone in x, clamped into the grid
__device__ __forceinline__ int md_cell_of(const MdHeader& H, int a, double x) {
    const double u = floor((x - H.lo[a]) * H.inv_h);
    const int top = H.n[a] - 1;
    return u <= 0.0 ? 0 : (u >= (double)top ? top : (int)u);
}

__global__ __launch_bounds__(kMdThreads) void k_md_stats(const float* __restrict__ tris, int n_faces, double* __restrict__ stat) {
    __shared__ double red[7][kMdThreads];
    const int t = threadIdx.x;
    double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300}, ext = 0.0;
    bool bad = false;
    for (int f = blockIdx.x * kMdThreads + t; f < n_faces; f += kMdStatBlocks * kMdThreads) {
        const float* v = tris + (size_t)f * 9;
        double e = 0.0;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double x0 = (double)v[c], x1 = (double)v[3 + c], x2 = (double)v[6 + c];
            bad = bad || !(fabs(x0) <= kMdFltMax) || !(fabs(x1) <= kMdFltMax) || !(fabs(x2) <= kMdFltMax);
            const double mn = fmin(x0, fmin(x1, x2)), mx = fmax(x0, fmax(x1, x2));
            lo[c] = fmin(lo[c], mn);
            hi[c] = fmax(hi[c], mx);
            e = fmax(e, mx - mn);
        }
        ext += e;
    }
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        red[c][t] = lo[c];
        red[3 + c][t] = hi[c];
    }
    red[6][t] = bad ? nan : ext;
    __syncthreads();
    for (int s = kMdThreads / 2; s > 0; s >>= 1) {   // fixed tree: the same mesh gives the same cell size
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
    if (t < 7) stat[(size_t)blockIdx.x * 8 + t] = red[t][0];
}

__global__ __launch_bounds__(kMdStatBlocks) void k_md_header(const double* __restrict__ stat, int n_faces, int cap_cells,
                                                             MdHeader* __restrict__ hdr) {
    __shared__ double red[7][kMdStatBlocks];
    const int t = threadIdx.x;
#pragma unroll
    for (int c = 0; c < 7; ++c) red[c][t] = stat[(size_t)t * 8 + c];
    __syncthreads();
    for (int s = kMdStatBlocks / 2; s > 0; s >>= 1) {
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
    MdHeader H;
    double side = 0.0;
    for (int c = 0; c < 3; ++c) {
        H.lo[c] = red[c][0];
        H.hi[c] = red[3 + c][0];
        side = fmax(side, H.hi[c] - H.lo[c]);
    }
    const double ext_sum = red[6][0];
    H.status = (ext_sum == ext_sum) ? 0 : 1;   // NaN: some vertex is not finite
    double h = 2.0 * ext_sum / (double)n_faces;
    if (!(h > 0.0)) h = side / 16.0;           // every triangle is a point
    if (!(h > 0.0)) h = 1.0;                   // ... the same point
    h = fmax(h, side / (double)(kMdMaxSide - 1));
    if (H.status) {
        h = 1.0;
        for (int c = 0; c < 3; ++c) H.lo[c] = H.hi[c] = 0.0;
    }
    for (int it = 0; it < 256; ++it) {         // the cell budget: grow h until the grid fits
        double cells = 1.0;
        for (int c = 0; c < 3; ++c) {
            const double n = floor((H.hi[c] - H.lo[c]) / h) + 1.0;
            H.n[c] = (int)fmin(n, (double)kMdMaxSide);
            cells *= (double)H.n[c];
        }
        if (cells <= (double)cap_cells) break;
        h *= 1.25;
    }
    H.h = h;
    H.inv_h = 1.0 / h;
    H.n_cells = H.n[0] * H.n[1] * H.n[2];
    H.n_refs = 0;
    H.n_big = 0;
    *hdr = H;
}

// FILL false: counts per cell and the big list;  true: the references (cell_count counts DOWN to hand out the slots)
template <bool FILL>
__global__ __launch_bounds__(kMdThreads) void k_md_bin(const float* __restrict__ tris, int n_faces, MdHeader* __restrict__ hdr,
                                                       int* __restrict__ cell_count, const int* __restrict__ cell_base,
                                                       int* __restrict__ refs, int* __restrict__ big) {
    const int f = blockIdx.x * kMdThreads + threadIdx.x;
    if (f >= n_faces) return;
    const MdHeader H = *hdr;
    if (H.status) return;
    const float* v = tris + (size_t)f * 9;
    int c0[3], c1[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double x0 = (double)v[c], x1 = (double)v[3 + c], x2 = (double)v[6 + c];
        c0[c] = md_cell_of(H, c, fmin(x0, fmin(x1, x2)));
        c1[c] = md_cell_of(H, c, fmax(x0, fmax(x1, x2)));
    }
    const long long span = (long long)(c1[0] - c0[0] + 1) * (c1[1] - c0[1] + 1) * (c1[2] - c0[2] + 1);
    if (span > kMdSpan) {
        if (!FILL) {
            const int k = atomicAdd(&hdr->n_big, 1);   // k < n_faces: one slot per triangle at most
            big[k] = f;
        }
        return;
    }
    for (int z = c0[2]; z <= c1[2]; ++z)
        for (int y = c0[1]; y <= c1[1]; ++y)
            for (int x = c0[0]; x <= c1[0]; ++x) {
                const int cell = (z * H.n[1] + y) * H.n[0] + x;   // < n_cells <= cap_cells
                if (FILL) {
                    const int slot = atomicSub(&cell_count[cell], 1) - 1;   // >= 0: the count pass counted this reference
                    refs[cell_base[cell] + slot] = f;                       // < n_refs <= kMdSpan * n_faces
                } else {
                    atomicAdd(&cell_count[cell], 1);
                }
            }
}

// base[i] = sum of count[0 .. i) for i <= n_cells (n_cells read from the header), header.n_refs = the total.  One workgroup
// walks the cells in chunks of 4096 -- four consecutive cells per thread, so a wave reads 1 KB in one piece -- with the
// in-row prefix of k_mcubes (wave shuffles, then the waves' sums through LDS) and a running carry.  Header: MdHeader, or the
// point index's PdHeader (pointdist.hpp) -- anything with n_cells and n_refs.
template <class Header>
__global__ __launch_bounds__(1024) void k_md_scan(const int* __restrict__ count, Header* __restrict__ hdr, int* __restrict__ base) {
    __shared__ int wsum[16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = hdr->n_cells;
    int carry = 0;
    for (int c0 = 0; c0 < n; c0 += 4096) {   // n is uniform: every thread makes every trip
        const int i = c0 + tid * 4;
        int v[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = i + q < n ? count[i + q] : 0;
        const int s = (v[0] + v[1]) + (v[2] + v[3]);
        int inc = s;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int u = __shfl_up(inc, o);
            if (lane >= o) inc += u;
        }
        if (lane == 63) wsum[wave] = inc;
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < 16; ++w) {
            if (w < wave) before += wsum[w];
            total += wsum[w];
        }
        __syncthreads();
        int run = carry + before + inc - s;
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (i + q < n) {
                base[i + q] = run;
                run += v[q];
            }
        carry += total;
    }
    if (tid == 0) {
        base[n] = carry;
        hdr->n_refs = carry;
    }
}

// One axis of the Chebyshev distance transform: out(c) = min over c' on c's line along AXIS of max(in(c'), |c - c'|), where
// in = 0 / 255 from the occupancy for AXIS 0.  The walk outwards ends as soon as the offset reaches the best value so far.
// Header: MdHeader or PdHeader (n[3], n_cells).
template <int AXIS, class Header = MdHeader>
__global__ __launch_bounds__(kMdThreads) void k_md_dt(const Header* __restrict__ hdr, const int* __restrict__ cell_base,
                                                      const uint8_t* __restrict__ in, uint8_t* __restrict__ out) {
    const int cell = blockIdx.x * kMdThreads + threadIdx.x;
    const int nx = hdr->n[0], ny = hdr->n[1], n_cells = hdr->n_cells;
    if (cell >= n_cells) return;
    const int x = cell % nx, y = (cell / nx) % ny, z = cell / (nx * ny);
    const int pos = AXIS == 0 ? x : AXIS == 1 ? y : z;
    const int len = hdr->n[AXIS];
    const int stride = AXIS == 0 ? 1 : AXIS == 1 ? nx : nx * ny;
    auto value = [&](int c) -> int {
        if (AXIS == 0) return cell_base[c + 1] > cell_base[c] ? 0 : 255;
        return (int)in[c];
    };
    int best = value(cell);
    for (int k = 1; k < best; ++k) {
        int v = 255;
        if (pos - k >= 0) v = min(v, value(cell - k * stride));
        if (pos + k < len) v = min(v, value(cell + k * stride));
        best = min(best, max(v, k));
    }
    out[cell] = (uint8_t)best;
}

struct MdBest {
    double d2, wa, wb, wc;
    int face;
};

// pts [P][3] float32 -> d2 [P], face [P], closest [P][3] (or null), tested [P] (or null): point-triangle tests of the query
__global__ __launch_bounds__(kMdQueryThreads) void k_md_closest(const float* __restrict__ tris, const MdHeader* __restrict__ hdr,
                                                                const int* __restrict__ cell_base, const uint8_t* __restrict__ dt,
                                                                const int* __restrict__ refs, const int* __restrict__ big,
                                                                const float* __restrict__ pts, int n_pts, double* __restrict__ d2_out,
                                                                int* __restrict__ face_out, double* __restrict__ closest_out,
                                                                int* __restrict__ tested_out) {
#pragma clang fp contract(off)   // the per-triangle lines are k_mesh_query's, under its contraction setting
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_pts) return;
    const MdHeader H = *hdr;
    const D3 p = {(double)pts[(size_t)i * 3], (double)pts[(size_t)i * 3 + 1], (double)pts[(size_t)i * 3 + 2]};
    const double pa[3] = {p.x, p.y, p.z};
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    bool finite = true;
#pragma unroll
    for (int c = 0; c < 3; ++c) finite = finite && fabs(pa[c]) <= kMdFltMax;
    if (H.status || !finite) {
        d2_out[i] = nan;
        face_out[i] = -1;
        if (closest_out)
            for (int c = 0; c < 3; ++c) closest_out[(size_t)i * 3 + c] = nan;
        if (tested_out) tested_out[i] = 0;
        return;
    }
    double best = 1e300, bwa = 0.0, bwb = 0.0, bwc = 0.0;
    int bface = -1, tested = 0;
    auto test = [&](int f) {
        const float* v = tris + (size_t)f * 9;
        const D3 a = {(double)v[0], (double)v[1], (double)v[2]}, b = {(double)v[3], (double)v[4], (double)v[5]},
                 c = {(double)v[6], (double)v[7], (double)v[8]};
        double wa, wb, wc;
        closest_on_triangle(p, a, b, c, wa, wb, wc);
        const D3 cp = {wa * a.x + wb * b.x + wc * c.x, wa * a.y + wb * b.y + wc * c.y, wa * a.z + wb * b.z + wc * c.z};
        const D3 dv = dsub(p, cp);
        const double d2 = ddot(dv, dv);
        if (d2 < best || (d2 == best && f < bface)) {
            best = d2;
            bface = f;
            bwa = wa;
            bwb = wb;
            bwc = wc;
        }
        ++tested;
    };
    for (int k = 0; k < H.n_big; ++k) test(big[k]);
    if (H.n_refs > 0) {
        // the clamp onto the box, its cell, and what the clamp gives away
        double pc[3], slack[3], off2 = 0.0;
        int cp[3], rmax = 0;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            pc[a] = fmin(fmax(pa[a], H.lo[a]), H.hi[a]);
            const double o = pa[a] - pc[a];
            off2 += o * o;
            cp[a] = md_cell_of(H, a, pc[a]);
            rmax = max(rmax, max(cp[a], H.n[a] - 1 - cp[a]));
            // absolute slack of every bound along this axis: 2^-20 cells (cell_of rounds within 2^-40 of a cell) and 2^-45 of
            // the coordinates' magnitude (the bounds' own subtractions round within 2^-52 of it)
            slack[a] = H.h * 0x1p-20 + (fabs(H.lo[a]) + fabs(H.hi[a]) + fabs(pa[a])) * 0x1p-45;
        }
        const double keep = 1.0 - 0x1p-30;   // ... and of squaring and adding them
        // lower bound of |p - t| along axis a for every t of cell index c
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
                // only the slab of cells within sqrt(best) of the point can pass the gap tests below: the ring is clipped to
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
                        for (int k = e0; k < e1; ++k) test(refs[k]);
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
    d2_out[i] = best;
    face_out[i] = bface;
    if (closest_out) {
        if (bface >= 0) {
            const float* v = tris + (size_t)bface * 9;
            for (int c = 0; c < 3; ++c)
                closest_out[(size_t)i * 3 + c] = bwa * (double)v[c] + bwb * (double)v[3 + c] + bwc * (double)v[6 + c];
        } else {
            for (int c = 0; c < 3; ++c) closest_out[(size_t)i * 3 + c] = nan;
        }
    }
    if (tested_out) tested_out[i] = tested;
}

// ---- the scores (DESIGN.md "Geometry metrics on the device") ---------------------------------------------------------------
// unit normal of face f: cross product in float64 on the float32 vertices, normalised (NaN for a face without one)
__device__ __forceinline__ D3 md_face_normal(const float* __restrict__ tris, int f) {
#pragma clang fp contract(off)
    const float* v = tris + (size_t)f * 9;
    const D3 a = {(double)v[0], (double)v[1], (double)v[2]}, b = {(double)v[3], (double)v[4], (double)v[5]},
             c = {(double)v[6], (double)v[7], (double)v[8]};
    const D3 e1 = dsub(b, a), e2 = dsub(c, a);
    const D3 n = {e1.y * e2.z - e1.z * e2.y, e1.z * e2.x - e1.x * e2.z, e1.x * e2.y - e1.y * e2.x};
    const double len = sqrt((n.x * n.x + n.y * n.y) + n.z * n.z);
    return D3{n.x / len, n.y / len, n.z / len};
}

// cum[i] = sum over f <= i of the area of triangle f (half the norm of its float64 cross product), for area-weighted sampling.
// One workgroup in a fixed order (wave shuffles, the waves' sums through LDS, a running carry): the same soup gives the same
// bits, which a device-wide look-back scan does not promise for floating-point sums.
__global__ __launch_bounds__(1024) void k_md_area_cumsum(const float* __restrict__ tris, int n, double* __restrict__ cum) {
#pragma clang fp contract(off)
    __shared__ double wsum[16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double carry = 0.0;
    for (int c0 = 0; c0 < n; c0 += 1024) {   // n is uniform: every thread makes every trip
        const int i = c0 + tid;
        double area = 0.0;
        if (i < n) {
            const float* v = tris + (size_t)i * 9;
            const D3 a = {(double)v[0], (double)v[1], (double)v[2]}, b = {(double)v[3], (double)v[4], (double)v[5]},
                     c = {(double)v[6], (double)v[7], (double)v[8]};
            const D3 e1 = dsub(b, a), e2 = dsub(c, a);
            const D3 x = {e1.y * e2.z - e1.z * e2.y, e1.z * e2.x - e1.x * e2.z, e1.x * e2.y - e1.y * e2.x};
            area = 0.5 * sqrt((x.x * x.x + x.y * x.y) + x.z * x.z);
        }
        double inc = area;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const double u = __shfl_up(inc, o);
            if (lane >= o) inc += u;
        }
        if (lane == 63) wsum[wave] = inc;
        __syncthreads();
        double before = 0.0, total = 0.0;
#pragma unroll
        for (int w = 0; w < 16; ++w) {
            if (w < wave) before += wsum[w];
            total += wsum[w];
        }
        __syncthreads();
        if (i < n) cum[i] = carry + (before + inc);
        carry += total;
    }
}

struct MdSide {
    const float* tris_x;     // the sampled mesh
    const int* sample_face;  // [n] face of tris_x each sample was drawn from
    const float* tris_y;     // the mesh the samples were queried against
    const double* d2;        // [n]
    const int* face;         // [n] closest face of tris_y
    int n, blocks;
};

// workgroup b < s0.blocks: samples of side 0, else of side 1 -> part[b][4] = sum d, sum d^2, sum c, max d  (fixed tree)
__global__ __launch_bounds__(kMdThreads) void k_md_metrics_part(MdSide s0, MdSide s1, double* __restrict__ part) {
#pragma clang fp contract(off)
    __shared__ double red[4][kMdThreads];
    const int t = threadIdx.x;
    const bool second = (int)blockIdx.x >= s0.blocks;
    const MdSide s = second ? s1 : s0;
    const int k = ((int)blockIdx.x - (second ? s0.blocks : 0)) * kMdThreads + t;
    double d = 0.0, d2 = 0.0, c = 0.0;
    if (k < s.n) {
        d2 = s.d2[k];
        d = sqrt(d2);
        const int g = s.face[k];
        if (g >= 0) {
            const D3 nx = md_face_normal(s.tris_x, s.sample_face[k]), ny = md_face_normal(s.tris_y, g);
            c = fabs((nx.x * ny.x + nx.y * ny.y) + nx.z * ny.z);
        } else {
            c = __longlong_as_double(0x7ff8000000000000ll);
        }
    }
    red[0][t] = d;
    red[1][t] = d2;
    red[2][t] = c;
    red[3][t] = d;
    __syncthreads();
    for (int w = kMdThreads / 2; w > 0; w >>= 1) {
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
}

// one workgroup: the partials of each side in index order (thread t takes t, t + 256, ...; then the fixed tree) -> out[9]
__global__ __launch_bounds__(kMdThreads) void k_md_metrics_finish(const double* __restrict__ part, int blocks0, int blocks1, int n0,
                                                                  int n1, double* __restrict__ out) {
#pragma clang fp contract(off)
    __shared__ double red[4][kMdThreads];
    __shared__ double tot[2][4];
    const int t = threadIdx.x;
    for (int side = 0; side < 2; ++side) {
        const double* p = part + (size_t)(side ? blocks0 : 0) * 4;
        const int nb = side ? blocks1 : blocks0;
        double a[4] = {0.0, 0.0, 0.0, 0.0};
        for (int k = t; k < nb; k += kMdThreads) {
            a[0] += p[(size_t)k * 4];
            a[1] += p[(size_t)k * 4 + 1];
            a[2] += p[(size_t)k * 4 + 2];
            const double v = p[(size_t)k * 4 + 3];
            a[3] = (a[3] != a[3] || v != v) ? a[3] + v : fmax(a[3], v);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) red[q][t] = a[q];
        __syncthreads();
        for (int w = kMdThreads / 2; w > 0; w >>= 1) {
            if (t < w) {
                red[0][t] += red[0][t + w];
                red[1][t] += red[1][t + w];
                red[2][t] += red[2][t + w];
                const double u = red[3][t], v = red[3][t + w];
                red[3][t] = (u != u || v != v) ? u + v : fmax(u, v);
            }
            __syncthreads();
        }
        if (t < 4) tot[side][t] = red[t][0];
        __syncthreads();
    }
    if (t != 0) return;
    const double na = (double)n0, nb = (double)n1;
    const double acc = tot[0][0] / na, comp = tot[1][0] / nb;
    out[0] = acc;
    out[1] = comp;
    out[2] = 0.5 * (acc + comp);
    out[3] = 0.5 * (tot[0][1] / na + tot[1][1] / nb);
    out[4] = 0.5 * (tot[0][2] / na + tot[1][2] / nb);
    out[5] = tot[0][3];
    out[6] = tot[1][3];
    out[7] = na;
    out[8] = nb;
}

}  // namespace
