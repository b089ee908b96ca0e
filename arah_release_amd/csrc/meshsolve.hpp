// meshsolve.hpp -- linear systems with the cotangent operator of an indexed mesh, solved on the device: Jacobi-preconditioned
// conjugate gradients in float64 over the neighbour CSR of meshadj.hpp and the weights of meshlaplace.hpp, for up to 32 independent
// columns.  What implicit smoothing (M + t S) p' = M p and harmonic extension stand on.
//
// Reference: none in its tree (its users take sparse solves from scipy / libigl; none is a dependency of this project).
// The rule is meshing.laplacian_solve, restated here once.  For every SOLVED vertex v and every column
//
//     mass_coef (area_v x_v) - stiff_coef (sum over v's USABLE entries of w (x_n - x_v)) = rhs_v,       x = x0 at every other vertex.
//
//   * live_v: the row x0[v] is finite in every column.  The entry (v, n) is USABLE when its weight is finite and live_n: decided
//     once, from x0.  dS_v = the sum of the usable weights of v in ascending neighbour id, from 0; a_v = area_v, and +0 when
//     mass_coef is 0 (the area is not looked at then); d_v = mass_coef a_v + stiff_coef dS_v;
//   * the class of v, the first that applies: 1 pinned, 2 not live, 3 a rhs row that is not finite, 4 mass_coef != 0 and area_v
//     not finite and > 0, 5 d_v not finite and > 0; otherwise 0, SOLVED.  counts[class] counts them; the others are HELD;
//   * Op(y)_v = mass_coef (a_v y_v) - stiff_coef acc on solved rows, acc = the sum over the usable entries in ascending neighbour
//     id, from 0, of w (y_n - y_v); +0 on held rows.  r, z, p, q are +0 on held rows throughout;
//   * <u, v> = the tree of meshquadric.hpp over the V products u_i v_i as ONE segment: a workgroup's tree over each aligned block
//     of 256 vertices (mq_group_tree), then the same tree over the blocks' sums -- which is that same tree;
//   * start: r = rhs - Op(x0), z = r / d, p = z, rz = <r, z>, rr = <r, r>, r0 = rr, thr = (tol tol) r0; status 2 (breakdown) when
//     r0 is not finite, else 1 (converged, 0 iterations) when rr <= thr;
//   * step of a column with status 0: q = Op(p), pq = <p, q>; pq not finite or not > 0: status 2, nothing else changes;
//     alpha = rz / pq, x = x + alpha p, r = r - alpha q, z = r / d, rz' = <r, z>, rr = <r, r>, iters += 1; rr <= thr: status 1;
//     otherwise beta = rz' / rz, p = z + beta p, rz = rz'.
//
// A step is FOUR launches, and its seams are kernel boundaries:
//
//   k_mz_op          (blocks of 256 vertices) x (columns): q = Op(p) by a gather -- a vertex's own lane writes its own row --, the
//                    block's tree over p q, one partial per block.  The direction is not stored by the step that computes beta:
//                    p = z + beta p of the step before is formed here on the fly, for the vertex and for its neighbours, from the
//                    stored z and p, which nobody writes in this launch.  That saves the step a fifth launch.
//   k_mz_fin_pq      one workgroup per column over the partials: pq, the breakdown test, alpha
//   k_mz_update      the same grid: the vertex's own p once more (the same operations, the same bits), now stored; x, r, z; the
//                    block's trees over r z and r r
//   k_mz_fin_rr      one workgroup per column: rz', rr, iters, the convergence test, beta
//
// Two seams are needed by the two inner products, whose results every vertex needs before it goes on; the finishes are launches of
// their own because only a kernel boundary orders the partials of all workgroups before their reader (no grid-wide barrier, no
// counter of finished workgroups, no spin-wait).  The scalars and the statuses of the columns live on the device; every kernel
// reads the status of its column first and does nothing for a stopped column, so a stopped column's arrays never change again
// and the steps left in a batch cost four empty launches.  No floating-point atomics anywhere; integer atomics for the counts of
// the classes only.  weight / nbr_start / nbr are the caller's: rows are clamped to the arrays, ids are tested before they are
// followed.  Workgroups synchronise by __syncthreads from workgroup-uniform control flow only; every loop ends by an argument of
// its own, stated at the loop.  `#pragma clang fp contract(off)` stands in EVERY function that does arithmetic.
// The cut into launches, the grid (a workgroup per block AND column, so that a tree has one or two rows) and Jacobi against no
// preconditioner are unmeasured choices.
#pragma once

constexpr int kMzMaxVerts = 1 << 24;              // 256 blocks of 256 blocks of 256 vertices: the finish is two more levels of the tree
constexpr int kMzMaxChannels = kMlMaxChannels;
constexpr unsigned kMzDead = 0x80u;               // bit 7 of MzState::cls: the vertex is not live, its entries are not usable
constexpr int kMzCounts = 8;                      // counts[0 .. 5] by class, counts[6], counts[7] = 0
enum { kMzRz = 0, kMzRr, kMzR0, kMzThr, kMzAlpha, kMzBeta, kMzColDoubles };   // rows of MzState::col, kMzMaxChannels wide
enum { kMzStatus = 0, kMzIters, kMzDir, kMzColInts };                         // rows of MzState::icol
static_assert(kImeshThreads == 256 && (long long)kImeshThreads * kImeshThreads * kImeshThreads == kMzMaxVerts, "the levels of the finish");

struct MzState {                                  // the scratch of a solve (carve_solve)
    double *d, *r, *z, *p, *q;                    // d [V]; r, z, p, q [C][V], column by column: neighbouring lanes, neighbouring words
    double* part;                                 // [2][C][blocks]: the blocks' sums of one or two inner products
    double* col;                                  // [kMzColDoubles][32]
    int *icol, *counts;                           // [kMzColInts][32], [kMzCounts]
    unsigned char *cls, *live;                    // [V] the class, with bit 7 (kMzDead) for a vertex that is not live; [V] live
};

struct MzMesh {                                   // the operator
    const double *weight, *area;
    const int *nbr_start, *nbr;
    int n_verts, n_ch, n_blocks;
    long long n_rows;
    double mass_coef, stiff_coef;
};

struct MzRow {
    long long es, ee;
};

__device__ __forceinline__ MzRow mz_row(const MzMesh& m, long long v) {
    MzRow r;
    r.es = min(max((long long)m.nbr_start[v], 0ll), m.n_rows);
    r.ee = min(max((long long)m.nbr_start[v + 1], r.es), m.n_rows);
    return r;
}

__device__ __forceinline__ double mz_area(const MzMesh& m, long long v) { return m.mass_coef != 0.0 ? m.area[v] : 0.0; }

// ---- begin 1: live[v] -------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kImeshThreads) void k_mz_live(const double* __restrict__ x0, int n_verts, int n_ch,
                                                           unsigned char* __restrict__ live) {
    const long long step = (long long)gridDim.x * blockDim.x;
    // terminates: n_verts - v strictly decreases (step >= 1) and the loop ends when it reaches 0
    for (long long v = (long long)blockIdx.x * blockDim.x + threadIdx.x; v < n_verts; v += step) {
        bool ok = true;
        for (int c = 0; c < n_ch; ++c) ok = ok && isfinite(x0[(size_t)v * n_ch + c]);   // terminates: n_ch - c strictly decreases
        live[v] = ok ? 1 : 0;
    }
}

// ---- begin 2: the usable entries, d and the class of every vertex -----------------------------------------------------------------
__global__ __launch_bounds__(kImeshThreads) void k_mz_class(MzMesh m, const double* __restrict__ rhs,
                                                            const unsigned char* __restrict__ pinned, MzState st) {
#pragma clang fp contract(off)
    const long long step = (long long)gridDim.x * blockDim.x, end = ((long long)m.n_verts + 63) & ~63ll;
    int tally[6] = {0, 0, 0, 0, 0, 0};
    // terminates: end - v strictly decreases (step >= 1); the vertex count is rounded up to whole waves so that every lane reaches
    // the reductions below
    for (long long v = (long long)blockIdx.x * blockDim.x + threadIdx.x; v < end; v += step) {
        if (v >= m.n_verts) continue;
        const MzRow row = mz_row(m, v);
        double dS = 0.0;
        for (long long k = row.es; k < row.ee; ++k) {   // terminates: ee - k strictly decreases
            const int n = m.nbr[k];
            const double w = m.weight[k];
            if ((unsigned)n < (unsigned)m.n_verts && isfinite(w) && st.live[n]) dS = dS + w;   // n is tested before it is followed
        }
        bool rhs_ok = true;
        for (int c = 0; c < m.n_ch; ++c) rhs_ok = rhs_ok && isfinite(rhs[(size_t)v * m.n_ch + c]);   // terminates: n_ch - c decreases
        const double a = mz_area(m, v);
        const double d = m.mass_coef * a + m.stiff_coef * dS;
        const int cls = (pinned && pinned[v])                              ? 1
                        : !st.live[v]                                     ? 2
                        : !rhs_ok                                         ? 3
                        : (m.mass_coef != 0.0 && !(isfinite(a) && a > 0.0)) ? 4
                        : !(isfinite(d) && d > 0.0)                       ? 5
                                                                          : 0;
        st.d[v] = d;
        st.cls[v] = (unsigned char)(cls | (st.live[v] ? 0u : kMzDead));
#pragma unroll
        for (int k = 0; k < 6; ++k) tally[k] += cls == k;
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) tally[k] += __shfl_down(tally[k], o);
        if ((threadIdx.x & 63) == 0 && tally[k]) atomicAdd(&st.counts[k], tally[k]);
    }
}

// the block's sums of NQ products, by the whole workgroup from uniform control flow: -> part[q][c][blk]
template <int NQ>
__device__ __forceinline__ void mz_block_sums(const MzMesh& m, double (*t)[kImeshThreads], const double prod[NQ], double* __restrict__ part) {
    const int tid = (int)threadIdx.x, blk = (int)blockIdx.x, c = (int)blockIdx.y;
#pragma unroll
    for (int q = 0; q < NQ; ++q) t[q][tid] = prod[q];
    mq_group_tree<NQ>(t, min(kImeshThreads, m.n_verts - blk * kImeshThreads));   // begins and ends with a barrier
    if (tid == 0) {
#pragma unroll
        for (int q = 0; q < NQ; ++q) part[((size_t)q * m.n_ch + c) * m.n_blocks + blk] = t[q][0];
    }
}

// the tree over the n_blocks sums of column c, by one workgroup from uniform control flow: chunks of 256 blocks, then the chunks'
// sums (n_blocks <= 2^16, so there are at most 256 of them).  No blocks: +0
template <int NQ>
__device__ __forceinline__ void mz_finish(const double* __restrict__ part, int c, int n_ch, int n_blocks, double (*t)[kImeshThreads],
                                          double (*lvl)[kImeshThreads], double out[NQ]) {
    const int tid = (int)threadIdx.x, n_chunks = (n_blocks + kImeshThreads - 1) / kImeshThreads;
    // terminates: n_chunks - j strictly decreases to 0; j and every bound are the same for all threads, so all reach every barrier
    for (int j = 0; j < n_chunks; ++j) {
        const int i = j * kImeshThreads + tid;
        if (i < n_blocks) {
#pragma unroll
            for (int q = 0; q < NQ; ++q) t[q][tid] = part[((size_t)q * n_ch + c) * n_blocks + i];
        }
        mq_group_tree<NQ>(t, min(kImeshThreads, n_blocks - j * kImeshThreads));
        if (tid < NQ) lvl[tid][j] = t[tid][0];
        __syncthreads();   // t is free for the next chunk, lvl[.][j] is written
    }
    if (tid < n_chunks) {
#pragma unroll
        for (int q = 0; q < NQ; ++q) t[q][tid] = lvl[q][tid];
    }
    mq_group_tree<NQ>(t, n_chunks);
#pragma unroll
    for (int q = 0; q < NQ; ++q) out[q] = n_chunks > 0 ? t[q][0] : 0.0;
}

// ---- begin 3: x = x0; r = rhs - Op(x0), z = r / d, p = z, q = 0; the blocks' sums of r z and r r --------------------------------------
__global__ __launch_bounds__(kImeshThreads) void k_mz_start(MzMesh m, const double* __restrict__ rhs, const double* __restrict__ x0,
                                                            double* __restrict__ x, MzState st) {
#pragma clang fp contract(off)
    __shared__ double t[2][kImeshThreads];
    const int c = (int)blockIdx.y;
    const long long v = (long long)blockIdx.x * kImeshThreads + threadIdx.x;
    double rv = 0.0, zv = 0.0;
    if (v < m.n_verts) {
        const size_t at = (size_t)v * m.n_ch + c;
        const double xv = x0[at];
        x[at] = xv;
        const MzRow row = mz_row(m, v);
        if (st.cls[v] == 0) {
            double acc = 0.0;
            for (long long k = row.es; k < row.ee; ++k) {   // terminates: ee - k strictly decreases
                const int n = m.nbr[k];
                if ((unsigned)n >= (unsigned)m.n_verts) continue;   // nbr is the caller's: never followed out of bounds
                const double w = m.weight[k];
                if (!isfinite(w) || (st.cls[n] & kMzDead)) continue;
                acc = acc + w * (x0[(size_t)n * m.n_ch + c] - xv);
            }
            const double op = m.mass_coef * (mz_area(m, v) * xv) - m.stiff_coef * acc;
            rv = rhs[at] - op;
            zv = rv / st.d[v];
        }
        const size_t i = (size_t)c * m.n_verts + v;
        st.r[i] = rv;
        st.z[i] = zv;
        st.p[i] = zv;
        st.q[i] = 0.0;
    }
    const double prod[2] = {rv * zv, rv * rv};
    mz_block_sums<2>(m, t, prod, st.part);
}

// ---- begin 4: the scalars of every column ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(kImeshThreads) void k_mz_fin_start(int n_ch, int n_blocks, double tol, MzState st) {
#pragma clang fp contract(off)
    __shared__ double t[2][kImeshThreads], lvl[2][kImeshThreads];
    const int c = (int)blockIdx.x;
    double s[2];
    mz_finish<2>(st.part, c, n_ch, n_blocks, t, lvl, s);
    if (threadIdx.x == 0) {
        const double r0 = s[1];
        st.col[kMzRz * kMzMaxChannels + c] = s[0];
        st.col[kMzRr * kMzMaxChannels + c] = r0;
        st.col[kMzR0 * kMzMaxChannels + c] = r0;
        const double thr = (tol * tol) * r0;
        st.col[kMzThr * kMzMaxChannels + c] = thr;
        st.col[kMzAlpha * kMzMaxChannels + c] = 0.0;
        st.col[kMzBeta * kMzMaxChannels + c] = 0.0;
        st.icol[kMzStatus * kMzMaxChannels + c] = !isfinite(r0) ? 2 : r0 <= thr ? 1 : 0;
        st.icol[kMzIters * kMzMaxChannels + c] = 0;
        st.icol[kMzDir * kMzMaxChannels + c] = 0;
    }
}

// p of this step at row i of column c: the stored p before the first step of the column, z + beta p of the step before afterwards
__device__ __forceinline__ double mz_dir(const MzState& st, size_t i, bool dir, double beta) {
#pragma clang fp contract(off)
    return dir ? st.z[i] + beta * st.p[i] : st.p[i];
}

// ---- step 1: q = Op(p); the blocks' sums of p q -------------------------------------------------------------------------------------
__global__ __launch_bounds__(kImeshThreads) void k_mz_op(MzMesh m, MzState st) {
#pragma clang fp contract(off)
    __shared__ double t[1][kImeshThreads];
    const int c = (int)blockIdx.y;
    if (st.icol[kMzStatus * kMzMaxChannels + c] != 0) return;   // the whole workgroup: the column has stopped
    const bool dir = st.icol[kMzDir * kMzMaxChannels + c] != 0;
    const double beta = st.col[kMzBeta * kMzMaxChannels + c];
    const long long v = (long long)blockIdx.x * kImeshThreads + threadIdx.x;
    double prod[1] = {0.0};
    if (v < m.n_verts && st.cls[v] == 0) {
        const size_t base = (size_t)c * m.n_verts, i = base + v;
        const double pv = mz_dir(st, i, dir, beta);
        const MzRow row = mz_row(m, v);
        double acc = 0.0;
        for (long long k = row.es; k < row.ee; ++k) {   // terminates: ee - k strictly decreases
            const int n = m.nbr[k];
            if ((unsigned)n >= (unsigned)m.n_verts) continue;   // nbr is the caller's: never followed out of bounds
            const double w = m.weight[k];
            const unsigned cn = st.cls[n];
            if (!isfinite(w) || (cn & kMzDead)) continue;
            const double pn = cn == 0 ? mz_dir(st, base + n, dir, beta) : 0.0;
            acc = acc + w * (pn - pv);
        }
        const double qv = m.mass_coef * (mz_area(m, v) * pv) - m.stiff_coef * acc;
        st.q[i] = qv;
        prod[0] = pv * qv;
    }
    mz_block_sums<1>(m, t, prod, st.part);
}

// ---- step 2: pq, the breakdown test, alpha ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kImeshThreads) void k_mz_fin_pq(int n_ch, int n_blocks, MzState st) {
#pragma clang fp contract(off)
    __shared__ double t[1][kImeshThreads], lvl[1][kImeshThreads];
    const int c = (int)blockIdx.x;
    if (st.icol[kMzStatus * kMzMaxChannels + c] != 0) return;   // the whole workgroup
    double s[1];
    mz_finish<1>(st.part, c, n_ch, n_blocks, t, lvl, s);
    if (threadIdx.x == 0) {
        const double pq = s[0];
        if (!(isfinite(pq) && pq > 0.0))
            st.icol[kMzStatus * kMzMaxChannels + c] = 2;
        else
            st.col[kMzAlpha * kMzMaxChannels + c] = st.col[kMzRz * kMzMaxChannels + c] / pq;
    }
}

// ---- step 3: p stored; x = x + alpha p, r = r - alpha q, z = r / d; the blocks' sums of r z and r r ----------------------------------
__global__ __launch_bounds__(kImeshThreads) void k_mz_update(MzMesh m, double* __restrict__ x, MzState st) {
#pragma clang fp contract(off)
    __shared__ double t[2][kImeshThreads];
    const int c = (int)blockIdx.y;
    if (st.icol[kMzStatus * kMzMaxChannels + c] != 0) return;   // the whole workgroup: stopped, or broken down in this step
    const bool dir = st.icol[kMzDir * kMzMaxChannels + c] != 0;
    const double beta = st.col[kMzBeta * kMzMaxChannels + c], alpha = st.col[kMzAlpha * kMzMaxChannels + c];
    const long long v = (long long)blockIdx.x * kImeshThreads + threadIdx.x;
    double prod[2] = {0.0, 0.0};
    if (v < m.n_verts && st.cls[v] == 0) {
        const size_t i = (size_t)c * m.n_verts + v, at = (size_t)v * m.n_ch + c;
        const double pv = mz_dir(st, i, dir, beta);
        st.p[i] = pv;
        x[at] = x[at] + alpha * pv;
        const double rv = st.r[i] - alpha * st.q[i];
        const double zv = rv / st.d[v];
        st.r[i] = rv;
        st.z[i] = zv;
        prod[0] = rv * zv;
        prod[1] = rv * rv;
    }
    mz_block_sums<2>(m, t, prod, st.part);
}

// ---- step 4: rz', rr, iters, the convergence test, beta ----------------------------------------------------------------------------
__global__ __launch_bounds__(kImeshThreads) void k_mz_fin_rr(int n_ch, int n_blocks, MzState st) {
#pragma clang fp contract(off)
    __shared__ double t[2][kImeshThreads], lvl[2][kImeshThreads];
    const int c = (int)blockIdx.x;
    if (st.icol[kMzStatus * kMzMaxChannels + c] != 0) return;   // the whole workgroup
    double s[2];
    mz_finish<2>(st.part, c, n_ch, n_blocks, t, lvl, s);
    if (threadIdx.x == 0) {
        st.col[kMzRr * kMzMaxChannels + c] = s[1];
        st.icol[kMzIters * kMzMaxChannels + c] += 1;
        if (s[1] <= st.col[kMzThr * kMzMaxChannels + c]) {
            st.icol[kMzStatus * kMzMaxChannels + c] = 1;
        } else {
            st.col[kMzBeta * kMzMaxChannels + c] = s[0] / st.col[kMzRz * kMzMaxChannels + c];
            st.col[kMzRz * kMzMaxChannels + c] = s[0];
            st.icol[kMzDir * kMzMaxChannels + c] = 1;
        }
    }
}

// ---- what the caller reads: iters, status, rr, r0 [C], counts [8], classes [V]; a null output is skipped ----------------------------
__global__ __launch_bounds__(kImeshThreads) void k_mz_report(int n_verts, int n_ch, MzState st, int* __restrict__ iters, int* __restrict__ status,
                                                             double* __restrict__ rr, double* __restrict__ r0, int* __restrict__ counts,
                                                             unsigned char* __restrict__ classes) {
    const long long step = (long long)gridDim.x * blockDim.x, first = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (first < n_ch) {
        const int c = (int)first;
        if (iters) iters[c] = st.icol[kMzIters * kMzMaxChannels + c];
        if (status) status[c] = st.icol[kMzStatus * kMzMaxChannels + c];
        if (rr) rr[c] = st.col[kMzRr * kMzMaxChannels + c];
        if (r0) r0[c] = st.col[kMzR0 * kMzMaxChannels + c];
    }
    if (first < kMzCounts && counts) counts[first] = st.counts[first];
    if (!classes) return;
    // terminates: n_verts - v strictly decreases (step >= 1) and the loop ends when it reaches 0
    for (long long v = first; v < n_verts; v += step) classes[v] = st.cls[v] & 0x7fu;
}
