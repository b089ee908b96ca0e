// metrics.hpp -- PSNR and SSIM of a rendered frame against its ground-truth image, on the device and without a host round
// trip.  The reference computes them on the host per validation frame (im2mesh/utils/eval.py:6-18): PSNR over the ray list,
// SSIM by skimage.metrics.structural_similarity (0.18.1: float64, 7 x 7 uniform window, sample covariance, the 3-pixel border
// cropped from the mean) on the crop cv2.boundingRect gives of the frame's ray mask.  Restated here in float64:
//   k_metrics_mse     one pass over the image: per workgroup the sum of (pred - gt)^2 over its masked pixels, their number and
//                     their bounding rectangle, to the scratch;
//   k_metrics_rect    one workgroup folds the per-workgroup rectangles into the frame's (scratch header).  (Measured: integer
//                     atomicMin / atomicMax from every workgroup on the four words instead cost 12 ns each, one after the other --
//                     49 of the pass's 50 us at 1002 x 1000);
//   k_metrics_ssim    a grid that covers the WHOLE image in tiles of kSsimTX x kSsimTY window centres anchored at the crop's
//                     first centre; the rectangle is read from device memory and tiles beyond the crop's centres write a zero
//                     partial and return.  Per tile and channel: the crop's pixels (3-pixel halo) widened to float64 in LDS, the
//                     five window sums separably (7 across, then 7 down), S per centre, the tile's sum in a fixed tree;
//   k_metrics_finish  one workgroup adds the per-workgroup / per-tile partials in index order and writes out[4], rect[5].
// No atomics anywhere: the same inputs give the same bits.  Nothing outside the crop is read by the SSIM pass,
// and a pixel outside the mask contributes nothing to the PSNR pass (it may hold NaN).
//
// LDS banking (8-byte reads are banked on 64 dwords and served per 32-lane half): every pass maps a 32-lane half onto ONE tile row
// -- lane l reads column l + k of a row of doubles, 32 consecutive 8-byte words = the 64 banks once -- so the reads are conflict-free
// for any row pitch and the pitches below carry no padding.  Included by arah_hip.hip.
#pragma once

namespace {

constexpr int kMetThreads = 256;
constexpr int kMsePix = 4;                                // pixels per thread of k_metrics_mse
constexpr int kMseBlockPix = kMetThreads * kMsePix;
constexpr int kSsimTX = 32, kSsimTY = 16;                 // window centres per tile
constexpr int kSsimWin = 7, kSsimHalo = 3;
constexpr int kSsimPX = kSsimTX + 2 * kSsimHalo;          // 38 pixels across
constexpr int kSsimPY = kSsimTY + 2 * kSsimHalo;          // 22 rows
constexpr size_t kMetHeaderBytes = 64;                    // int bounds[4] = min x, min y, max x, max y

struct MetricsScratch {
    int* bounds;
    double* mse_part;        // [n_mse_blocks]
    unsigned* cnt_part;      // [n_mse_blocks]
    int* bnd_part;           // [n_mse_blocks][4] min x, min y, max x, max y of the workgroup's masked pixels
    double* ssim_part;       // [tiles_y * tiles_x][3]
    int n_mse_blocks, tiles_x, tiles_y;
    size_t bytes;
};

inline MetricsScratch carve_metrics(void* base, int height, int width) {
    MetricsScratch m;
    const long long pixels = (long long)height * width;
    m.n_mse_blocks = (int)((pixels + kMseBlockPix - 1) / kMseBlockPix);
    m.tiles_x = (width + kSsimTX - 1) / kSsimTX;
    m.tiles_y = (height + kSsimTY - 1) / kSsimTY;
    char* p = reinterpret_cast<char*>(base);
    size_t off = 0;
    m.bounds = reinterpret_cast<int*>(p + off);
    off += kMetHeaderBytes;
    m.mse_part = reinterpret_cast<double*>(p + off);
    off += sizeof(double) * (size_t)m.n_mse_blocks;
    m.ssim_part = reinterpret_cast<double*>(p + off);
    off += sizeof(double) * 3 * (size_t)m.tiles_x * m.tiles_y;
    m.cnt_part = reinterpret_cast<unsigned*>(p + off);
    off += sizeof(unsigned) * (size_t)m.n_mse_blocks;
    m.bnd_part = reinterpret_cast<int*>(p + off);
    off += sizeof(int) * 4 * (size_t)m.n_mse_blocks;
    m.bytes = (off + 255) & ~(size_t)255;
    return m;
}

// sum of red[0 .. kMetThreads) in a fixed binary tree; the result is valid in thread 0
__device__ __forceinline__ double met_block_sum(double* red, double v) {
    const int t = threadIdx.x;
    red[t] = v;
    __syncthreads();
#pragma unroll
    for (int s = kMetThreads / 2; s > 0; s >>= 1) {
        if (t < s) red[t] += red[t + s];
        __syncthreads();
    }
    return red[0];
}

// Every in-bounds pixel is loaded and the mask selects (no data-dependent branch in front of the loads, so all of a thread's
// loads are in flight together); a pixel outside the mask contributes nothing, whatever it holds.
__global__ __launch_bounds__(kMetThreads) void k_metrics_mse(const float* __restrict__ pred, const float* __restrict__ gt,
                                                             const uint8_t* __restrict__ box_mask, int height, int width,
                                                             double* __restrict__ mse_part, unsigned* __restrict__ cnt_part,
                                                             int* __restrict__ bnd_part) {
    __shared__ double red[kMetThreads];
    __shared__ int ired[5][kMetThreads];
    const int t = threadIdx.x;
    const unsigned pixels = (unsigned)height * (unsigned)width;      // <= 2^30 (checked by the caller)
    float a[kMsePix][3], b[kMsePix][3];
    bool in[kMsePix];
#pragma unroll
    for (int k = 0; k < kMsePix; ++k) {
        const unsigned p = blockIdx.x * (unsigned)kMseBlockPix + k * kMetThreads + t;
        const size_t q = (size_t)(p < pixels ? p : 0u) * 3;
        in[k] = p < pixels && box_mask[p < pixels ? p : 0u] != 0;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            a[k][c] = pred[q + c];
            b[k][c] = gt[q + c];
        }
    }
    double acc = 0.0;
    int cnt = 0, lo_x = 0x7fffffff, lo_y = 0x7fffffff, hi_x = -1, hi_y = -1;
#pragma unroll
    for (int k = 0; k < kMsePix; ++k) {
        const unsigned p = blockIdx.x * (unsigned)kMseBlockPix + k * kMetThreads + t;
        const int y = (int)(p / (unsigned)width), x = (int)(p - (unsigned)y * (unsigned)width);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double d = (double)a[k][c] - (double)b[k][c];
            acc += in[k] ? d * d : 0.0;
        }
        cnt += in[k] ? 1 : 0;
        lo_x = in[k] ? min(lo_x, x) : lo_x;
        hi_x = in[k] ? max(hi_x, x) : hi_x;
        lo_y = in[k] ? min(lo_y, y) : lo_y;
        hi_y = in[k] ? max(hi_y, y) : hi_y;
    }
    red[t] = acc;
    ired[0][t] = cnt;
    ired[1][t] = lo_x;
    ired[2][t] = lo_y;
    ired[3][t] = hi_x;
    ired[4][t] = hi_y;
    __syncthreads();
    for (int s = kMetThreads / 2; s > 0; s >>= 1) {      // one fixed tree for the sum, the count and the bounds
        if (t < s) {
            red[t] += red[t + s];
            ired[0][t] += ired[0][t + s];
            ired[1][t] = min(ired[1][t], ired[1][t + s]);
            ired[2][t] = min(ired[2][t], ired[2][t + s]);
            ired[3][t] = max(ired[3][t], ired[3][t + s]);
            ired[4][t] = max(ired[4][t], ired[4][t + s]);
        }
        __syncthreads();
    }
    if (t == 0) {
        mse_part[blockIdx.x] = red[0];
        cnt_part[blockIdx.x] = (unsigned)ired[0][0];
#pragma unroll
        for (int q = 0; q < 4; ++q) bnd_part[(size_t)blockIdx.x * 4 + q] = ired[1 + q][0];   // no masked pixel: (max, max, -1, -1)
    }
}

// one workgroup: bounds[4] = the rectangle of all workgroups' rectangles (max x < min x: the mask is empty)
__global__ __launch_bounds__(kMetThreads) void k_metrics_rect(const int* __restrict__ bnd_part, int n_mse_blocks,
                                                              int* __restrict__ bounds) {
    __shared__ int ired[4][kMetThreads];
    const int t = threadIdx.x;
    int lo_x = 0x7fffffff, lo_y = 0x7fffffff, hi_x = -1, hi_y = -1;
    for (int k = t; k < n_mse_blocks; k += kMetThreads) {
        lo_x = min(lo_x, bnd_part[(size_t)k * 4 + 0]);
        lo_y = min(lo_y, bnd_part[(size_t)k * 4 + 1]);
        hi_x = max(hi_x, bnd_part[(size_t)k * 4 + 2]);
        hi_y = max(hi_y, bnd_part[(size_t)k * 4 + 3]);
    }
    ired[0][t] = lo_x;
    ired[1][t] = lo_y;
    ired[2][t] = hi_x;
    ired[3][t] = hi_y;
    __syncthreads();
    for (int s = kMetThreads / 2; s > 0; s >>= 1) {
        if (t < s) {
            ired[0][t] = min(ired[0][t], ired[0][t + s]);
            ired[1][t] = min(ired[1][t], ired[1][t + s]);
            ired[2][t] = max(ired[2][t], ired[2][t + s]);
            ired[3][t] = max(ired[3][t], ired[3][t + s]);
        }
        __syncthreads();
    }
    if (t < 4) bounds[t] = ired[t][0];
}

// grid (tiles_x, tiles_y, 3 channels)
__global__ __launch_bounds__(kMetThreads) void k_metrics_ssim(const float* __restrict__ pred, const float* __restrict__ gt, int height,
                                                              int width, const int* __restrict__ bounds, double c1, double c2,
                                                              double* __restrict__ ssim_part) {
    __shared__ double px[kSsimPY][kSsimPX], py[kSsimPY][kSsimPX];     // the tile's pixels + halo, float64
    __shared__ double hs[5][kSsimPY][kSsimTX];                        // horizontal window sums of x, y, xx, yy, xy
    __shared__ double red[kMetThreads];
    const int t = threadIdx.x, ch = blockIdx.z;
    double* out = ssim_part + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 3 + ch;
    const int bx0 = bounds[0], by0 = bounds[1], bx1 = bounds[2], by1 = bounds[3];     // inclusive; max < min: empty mask
    const int cw = bx1 - bx0 + 1 - 2 * kSsimHalo, chh = by1 - by0 + 1 - 2 * kSsimHalo;  // window centres across / down
    const int ox = blockIdx.x * kSsimTX, oy = blockIdx.y * kSsimTY;                   // the tile's first centre, crop-relative - halo
    if (bx1 < bx0 || cw < 1 || chh < 1 || ox >= cw || oy >= chh) {                    // uniform over the workgroup
        if (t == 0) *out = 0.0;
        return;
    }
    // pixel (j, i) of the tile is crop pixel (ox + j, oy + i); beyond the crop: 0, never read from memory
    for (int k = t; k < kSsimPY * kSsimPX; k += kMetThreads) {
        const int i = k / kSsimPX, j = k - i * kSsimPX;
        const int gx = bx0 + ox + j, gy = by0 + oy + i;
        double a = 0.0, b = 0.0;
        if (gx <= bx1 && gy <= by1) {
            const size_t q = ((size_t)gy * width + gx) * 3 + ch;
            a = (double)pred[q];
            b = (double)gt[q];
        }
        px[i][j] = a;
        py[i][j] = b;
    }
    __syncthreads();
    for (int k = t; k < kSsimPY * kSsimTX; k += kMetThreads) {
        const int i = k / kSsimTX, j = k % kSsimTX;
        double sx = 0.0, sy = 0.0, sxx = 0.0, syy = 0.0, sxy = 0.0;
#pragma unroll
        for (int d = 0; d < kSsimWin; ++d) {
            const double a = px[i][j + d], b = py[i][j + d];
            sx += a;
            sy += b;
            sxx += a * a;
            syy += b * b;
            sxy += a * b;
        }
        hs[0][i][j] = sx;
        hs[1][i][j] = sy;
        hs[2][i][j] = sxx;
        hs[3][i][j] = syy;
        hs[4][i][j] = sxy;
    }
    __syncthreads();
    constexpr double inv_n = 1.0 / (kSsimWin * kSsimWin), cov_norm = (double)(kSsimWin * kSsimWin) / (kSsimWin * kSsimWin - 1);
    double acc = 0.0;
    for (int k = t; k < kSsimTY * kSsimTX; k += kMetThreads) {
        const int i = k / kSsimTX, j = k % kSsimTX;
        double s[5];
#pragma unroll
        for (int q = 0; q < 5; ++q) {
            double v = 0.0;
#pragma unroll
            for (int d = 0; d < kSsimWin; ++d) v += hs[q][i + d][j];
            s[q] = v * inv_n;
        }
        const double ux = s[0], uy = s[1];
        const double vx = cov_norm * (s[2] - ux * ux), vy = cov_norm * (s[3] - uy * uy), vxy = cov_norm * (s[4] - ux * uy);
        const double a1 = 2.0 * ux * uy + c1, a2 = 2.0 * vxy + c2, b1 = ux * ux + uy * uy + c1, b2 = vx + vy + c2;
        const double S = (a1 * a2) / (b1 * b2);
        if (ox + j < cw && oy + i < chh) acc += S;
    }
    const double sum = met_block_sum(red, acc);
    if (t == 0) *out = sum;
}

// one workgroup: partials added in index order (thread t takes t, t + 256, ...; then the fixed tree)
__global__ __launch_bounds__(kMetThreads) void k_metrics_finish(const int* __restrict__ bounds, const double* __restrict__ mse_part,
                                                                const unsigned* __restrict__ cnt_part, int n_mse_blocks,
                                                                const double* __restrict__ ssim_part, int n_tiles,
                                                                double* __restrict__ out, int* __restrict__ rect) {
    __shared__ double red[kMetThreads];
    __shared__ unsigned long long cred[kMetThreads];
    const int t = threadIdx.x;
    double m = 0.0;
    unsigned long long cnt = 0;
    for (int k = t; k < n_mse_blocks; k += kMetThreads) {
        m += mse_part[k];
        cnt += cnt_part[k];
    }
    cred[t] = cnt;
    const double se = met_block_sum(red, m);
    __syncthreads();
    for (int s = kMetThreads / 2; s > 0; s >>= 1) {
        if (t < s) cred[t] += cred[t + s];
        __syncthreads();
    }
    double ch_sum[3];
    for (int c = 0; c < 3; ++c) {
        double v = 0.0;
        for (int k = t; k < n_tiles; k += kMetThreads) v += ssim_part[(size_t)k * 3 + c];
        ch_sum[c] = met_block_sum(red, v);
        __syncthreads();
    }
    if (t != 0) return;
    const unsigned long long n = cred[0];
    const int bx0 = bounds[0], by0 = bounds[1], bx1 = bounds[2], by1 = bounds[3];
    const double nan = __longlong_as_double(0x7ff8000000000000ll), inf = __longlong_as_double(0x7ff0000000000000ll);
    int status = 0, w = 0, h = 0;
    if (n == 0) {
        status = 1;
    } else {
        w = bx1 - bx0 + 1;
        h = by1 - by0 + 1;
        if (w < kSsimWin || h < kSsimWin) status = 2;
    }
    const double mse = n ? se / (3.0 * (double)n) : nan;
    out[0] = n ? (mse == 0.0 ? inf : -10.0 * log10(mse)) : nan;
    if (status == 0) {
        const double centres = (double)(w - 2 * kSsimHalo) * (double)(h - 2 * kSsimHalo);
        out[1] = (ch_sum[0] / centres + ch_sum[1] / centres + ch_sum[2] / centres) / 3.0;
    } else {
        out[1] = nan;
    }
    out[2] = mse;
    out[3] = (double)n;
    rect[0] = n ? bx0 : 0;
    rect[1] = n ? by0 : 0;
    rect[2] = w;
    rect[3] = h;
    rect[4] = status;
}

}  // namespace
