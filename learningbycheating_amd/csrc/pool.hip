// Stem tail for gfx950: BatchNorm + ReLU + MaxPool2d(3,2,1) fused in one pass over
// the largest activation of the network (N x 80 x 192 x 64 for the RGB model), and
// the matching backward (max-pool scatter as a gather + ReLU mask + BatchNorm
// gradient reductions) in one pass.  reference: bird_view/models/resnet.py:104-106,
// 149-152.  The forward stores the arg-max tap (0..8, first maximum in row-major
// order, as torch does) per pooled element so the backward never re-scans windows.
#include "lbc_common.hpp"
#include "lbc_act.hpp"
#include "lbc_kernels.hpp"

namespace {

// Workgroup ids go round-robin over the 8 XCDs, each with an L2 of its own.  Both passes below re-read rows across workgroup boundaries
// (a 3 x 3 / 2 window shares an input row with the window below it; a pixel range shares pooled rows with the next range): with
// consecutive ranges on consecutive ids every shared row was fetched by two XCDs (PMC: 629 MB for the 503 MB forward input, 1041 MB for
// the backward's 693, profiles/r05_final_pmc_summary_bf16.txt).  Logical id = XCD-major: consecutive ranges sit on ONE XCD.
__device__ __forceinline__ unsigned xcd_major_block()
{
    const unsigned nwg = gridDim.x, b = blockIdx.x;
    const unsigned xcd = b & 7u, q = nwg >> 3, rr = nwg & 7u;
    return (xcd < rr ? xcd * (q + 1) : rr * (q + 1) + (xcd - rr) * q) + (b >> 3);
}

// A lane owns one 16-byte channel group of one output column and walks down kPoolRun output rows of one image: the input row
// under a window is the top row of the next window, so it is loaded and put through the affine once and carried in registers
// (six 16-byte loads per output vector where nine were, every input row read 1 + 1 / (2 kPoolRun) times), and the addresses
// advance by a row; the only divisions place the lane.  Lanes are numbered column group fastest, then run, then image, and
// workgroups take 256 consecutive lanes in XCD-major order.
constexpr int kPoolRun = 8;

template <typename T, typename IDX>
__global__ __launch_bounds__(256) void bn_relu_maxpool_fwd_k(PoolFwdArgs a)
{
    constexpr int V = Act<T>::kVec;          // 16-byte accesses: 4 f32 or 8 bf16 channels per thread
    using vec = typename Act<T>::vec;
    using PV = ParamVec<V>;
    const int OH = a.H / 2, OW = a.W / 2;
    const int cvn = a.C / V;
    const int lanes_row = OW * cvn, runs = (OH + kPoolRun - 1) / kPoolRun;
    // IDX = unsigned when the lane count of the launch fits 32 bits (lbc_bn_relu_maxpool_fwd): 64-bit divisions otherwise
    const IDX u = (IDX)xcd_major_block() * (IDX)256 + (IDX)threadIdx.x;
    if (u >= (IDX)((long long)a.N * runs * lanes_row)) return;
    const int sl = (int)(u % (IDX)lanes_row);
    const IDX t = u / (IDX)lanes_row;
    const int run = (int)(t % (IDX)runs), n = (int)(t / (IDX)runs);
    const int ox = sl / cvn, c = (sl - ox * cvn) * V;
    const int oy0 = run * kPoolRun;
    const int nrow = OH - oy0 < kPoolRun ? OH - oy0 : kPoolRun;
    const vec sc = PV::ld(a.scale + c), sh = PV::ld(a.shift + c);
    const vec ninf = PV::splat(-INFINITY);
    // of a window's taps only the row above output row 0 and the column left of output column 0 can lie outside (H and W are
    // even); those are loaded from a clamped, always valid address and enter as -inf, which never beats the running maximum
    const bool okl = ox > 0, okt = oy0 > 0;
    const size_t rowe = (size_t)a.W * a.C;
    const int col[3] = {okl ? -a.C : 0, 0, a.C};
    const T* src = static_cast<const T*>(a.y) + ((size_t)n * a.H + (size_t)(2 * oy0)) * rowe + (size_t)(2 * ox) * a.C + c;
    size_t o = (((size_t)n * OH + (size_t)oy0) * OW + (size_t)ox) * a.C + c;
    T* pout = static_cast<T*>(a.p);
    vec top[3];
    {
        const T* tp = src - (okt ? rowe : 0);
        typename Act<T>::raw raw[3];
#pragma unroll
        for (int s = 0; s < 3; ++s) raw[s] = Act<T>::ldr(tp + col[s]);
#pragma unroll
        for (int s = 0; s < 3; ++s) {
            vec v = Act<T>::cvt(raw[s]);
            v = v * sc + sh;
#pragma unroll
            for (int e = 0; e < V; ++e) top[s][e] = okt && (s > 0 || okl) ? fmaxf(v[e], 0.f) : -INFINITY;
        }
    }
    for (int r = 0; r < nrow; ++r) {
        typename Act<T>::raw raw[6];         // every load of the two new rows is requested before the first is used
#pragma unroll
        for (int q = 0; q < 6; ++q) raw[q] = Act<T>::ldr(src + (q / 3) * rowe + col[q % 3]);
        vec best = ninf;
        int bi[V];
#pragma unroll
        for (int e = 0; e < V; ++e) bi[e] = 0;
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {  // taps in row-major order, strict comparison: the first maximum wins
            vec z;
            if (tap < 3) {
                z = top[tap];
            } else {
                vec v = Act<T>::cvt(raw[tap - 3]);
                v = v * sc + sh;
#pragma unroll
                for (int e = 0; e < V; ++e) z[e] = tap % 3 > 0 || okl ? fmaxf(v[e], 0.f) : -INFINITY;
                if (tap >= 6) top[tap - 6] = z;
            }
#pragma unroll
            for (int e = 0; e < V; ++e)
                if (z[e] > best[e]) { best[e] = z[e]; bi[e] = tap; }
        }
        Act<T>::stv(pout + o, best);
        if (a.idx) {
#pragma unroll
            for (int q = 0; q < V / 4; ++q) {
                uchar4 w;
                w.x = (unsigned char)bi[4 * q]; w.y = (unsigned char)bi[4 * q + 1]; w.z = (unsigned char)bi[4 * q + 2]; w.w = (unsigned char)bi[4 * q + 3];
                reinterpret_cast<uchar4*>(a.idx + o)[q] = w;
            }
        }
        src += 2 * rowe;
        o += (size_t)OW * a.C;
    }
}

// Backward: for every stem-output element gather the pooled gradients whose arg-max
// is this element, apply the ReLU mask, store g and reduce (sum g, sum g*xhat).
template <typename T, typename IDX>      // IDX = unsigned when the pixel index fits 32 bits (64-bit divisions to place the lane's first pixel otherwise)
__global__ __launch_bounds__(256) void maxpool_relu_bwd_reduce_k(PoolBwdArgs a)
{
    constexpr int V = Act<T>::kVec;
    using vec = typename Act<T>::vec;
    using PV = ParamVec<V>;
    __shared__ __attribute__((aligned(16))) float red[2 * 256 * V];
    const T* dp = static_cast<const T*>(a.dp);
    const T* y = static_cast<const T*>(a.y);
    T* gout = static_cast<T*>(a.g);
    const int OH = a.H / 2, OW = a.W / 2;
    const int cvn = a.C / V;
    const int rl = 256 / cvn;
    const int cg = threadIdx.x % cvn;
    const int pl = threadIdx.x / cvn;
    const int c = cg * V;
    vec s1 = PV::splat(0.f), s2 = s1;
    if (pl < rl) {
        const vec sc = PV::ld(a.scale + c), sh = PV::ld(a.shift + c);
        const vec mean = PV::ld(a.mean + c), inv = PV::ld(a.invstd + c);
        const long long pixels = (long long)a.N * a.H * a.W;
        const long long p0 = (long long)xcd_major_block() * a.pix_per_block;
        long long p1 = p0 + a.pix_per_block;
        if (p1 > pixels) p1 = pixels;
        // (row, column, image) of the lane's pixel: placed once, then advanced by the lane stride
        int x = 0, yy = 0, n = 0;
        if (p0 + pl < p1) {
            const IDX pi = (IDX)(p0 + pl);
            x = (int)(pi % (IDX)a.W);
            const IDX t = pi / (IDX)a.W;
            yy = (int)(t % (IDX)a.H);
            n = (int)(t / (IDX)a.H);
        }
        for (long long p = p0 + pl; p < p1; p += rl) {
            vec g = PV::splat(0.f);
            const int oy0 = yy >> 1, oy1 = (yy + 1) >> 1;   // windows covering row y (equal when y is even)
            const int ox0 = x >> 1, ox1 = (x + 1) >> 1;
            // the two windows of the upper pooled row as a fixed pair with a validity flag, the two of the lower one under `rok`: a
            // pooled row serves the two or three rows under it, and an even row (or the last one) lies under one pooled row only.
            // The lanes of a wave mostly share a row, so the wave skips those loads and comparisons.  Every load is requested
            // before the first use (column 0 always exists; the second exists when it differs and lies inside).
            const bool rok = oy1 != oy0 && oy1 < OH, cok = ox1 != ox0 && ox1 < OW;
            const int oxw[2] = {ox0, cok ? ox1 : ox0};
            const int tx[2] = {x - (2 * ox0 - 1), x - (2 * ox1 - 1)};
            typename Act<T>::raw draw[4];
            uchar4 uraw[4][V / 4];
            const size_t orow = (size_t)(n * OH + oy0) * OW;
#pragma unroll
            for (int wv = 0; wv < 2; ++wv) {
                const size_t o = (orow + (size_t)oxw[wv]) * cvn + cg;
                draw[wv] = Act<T>::ldr(dp + o * V);
#pragma unroll
                for (int q = 0; q < V / 4; ++q) uraw[wv][q] = reinterpret_cast<const uchar4*>(a.idx)[o * (V / 4) + q];
            }
            if (rok) {
#pragma unroll
                for (int wv = 2; wv < 4; ++wv) {
                    const size_t o = (orow + (size_t)OW + (size_t)oxw[wv & 1]) * cvn + cg;
                    draw[wv] = Act<T>::ldr(dp + o * V);
#pragma unroll
                    for (int q = 0; q < V / 4; ++q) uraw[wv][q] = reinterpret_cast<const uchar4*>(a.idx)[o * (V / 4) + q];
                }
            }
            const typename Act<T>::raw yraw = Act<T>::ldr(y + (p * cvn + cg) * V);
            // in the order (oy0, ox0), (oy0, ox1), (oy1, ox0), (oy1, ox1)
            auto gather = [&](int wv, int tap) {
                const vec d = Act<T>::cvt(draw[wv]);
#pragma unroll
                for (int q = 0; q < V / 4; ++q) {
                    const uchar4 u = uraw[wv][q];
                    if (u.x == tap) g[4 * q] += d[4 * q];
                    if (u.y == tap) g[4 * q + 1] += d[4 * q + 1];
                    if (u.z == tap) g[4 * q + 2] += d[4 * q + 2];
                    if (u.w == tap) g[4 * q + 3] += d[4 * q + 3];
                }
            };
            const int ty = (yy - (2 * oy0 - 1)) * 3;
            gather(0, ty + tx[0]);
            gather(1, cok ? ty + tx[1] : 255);              // (255: no arg-max index matches)
            if (rok) {                                      // (yy - (2 oy1 - 1) = 0: the top row of the lower windows)
                gather(2, tx[0]);
                gather(3, cok ? tx[1] : 255);
            }
            const vec v = Act<T>::cvt(yraw);
            const vec z = v * sc + sh;
#pragma unroll
            for (int e = 0; e < V; ++e) g[e] = z[e] > 0.f ? g[e] : 0.f;
            Act<T>::stv(gout + (p * cvn + cg) * V, g);
            s1 += g;
            s2 += g * (v - mean) * inv;
            x += rl;
            while (x >= a.W) {
                x -= a.W;
                if (++yy == a.H) { yy = 0; ++n; }
            }
        }
    }
    PV::st(red + threadIdx.x * V, s1);
    PV::st(red + (256 + threadIdx.x) * V, s2);
    __syncthreads();
    if (threadIdx.x < cvn) {
        vec t1 = PV::splat(0.f), t2 = t1;
        for (int k = 0; k < rl; ++k) {
            t1 += PV::ld(red + (k * cvn + threadIdx.x) * V);
            t2 += PV::ld(red + (256 + k * cvn + threadIdx.x) * V);
        }
        float* dst = a.partial + (size_t)blockIdx.x * 2 * a.C;
        PV::st(dst + c, t1);
        PV::st(dst + a.C + c, t2);
    }
}

}  // namespace

int lbc_bn_relu_maxpool_fwd(const PoolFwdArgs& a, hipStream_t s)
{
    LBC_REQUIRE(a.C % 8 == 0 && a.H % 2 == 0 && a.W % 2 == 0, "maxpool: bad shape");
    const long long total = (long long)a.N * (a.H / 2) * (a.W / 2) * (a.C / 4);
    const int OH = a.H / 2;
    const long long lanes = (long long)a.N * ((OH + kPoolRun - 1) / kPoolRun) * (a.W / 2) * (a.C / (a.act_bf16 ? 8 : 4));
    const long long blocks = (lanes + 255) / 256;
    LBC_REQUIRE(blocks < (1ll << 31), "maxpool: too large");
    LbcProfScope prof("bn_relu_maxpool_fwd", 0.0, (a.act_bf16 ? 2.0 : 4.0) * total * 4 * (4.0 + 1.0) + total * 4.0, s);
    const bool small = lanes + 256 < (1ll << 32);
#define LBC_K(T, g)                                                                                                          \
    do {                                                                                                                     \
        if (small) hipLaunchKernelGGL((bn_relu_maxpool_fwd_k<T, unsigned>), dim3((unsigned)(g)), dim3(256), 0, s, a);        \
        else       hipLaunchKernelGGL((bn_relu_maxpool_fwd_k<T, long long>), dim3((unsigned)(g)), dim3(256), 0, s, a);       \
    } while (0)
    LBC_DISPATCH_ACT(a.act_bf16, LBC_K, blocks);
#undef LBC_K
    return lbc_check_launch("bn_relu_maxpool_fwd");
}

int lbc_pool_bwd_rows(int N, int H, int W, int C) { return lbc_chan_reduce_rows((long long)N * H * W, C); }

int lbc_maxpool_relu_bwd_reduce(PoolBwdArgs a, hipStream_t s)
{
    LBC_REQUIRE(a.C % 8 == 0 && a.C / 4 <= 256, "maxpool_bwd: bad C");
    const long long pixels = (long long)a.N * a.H * a.W;
    const int rows = lbc_pool_bwd_rows(a.N, a.H, a.W, a.C);
    a.pix_per_block = (pixels + rows - 1) / rows;
    LbcProfScope prof("maxpool_relu_bwd_reduce", 0.0, (a.act_bf16 ? 2.0 : 4.0) * (double)pixels * a.C * (2.0 + 0.25) + (double)pixels * a.C * 0.25, s);
    const bool small = pixels < (1ll << 31);
#define LBC_K(T, g)                                                                                                              \
    do {                                                                                                                         \
        if (small) hipLaunchKernelGGL((maxpool_relu_bwd_reduce_k<T, unsigned>), dim3((unsigned)(g)), dim3(256), 0, s, a);        \
        else       hipLaunchKernelGGL((maxpool_relu_bwd_reduce_k<T, long long>), dim3((unsigned)(g)), dim3(256), 0, s, a);       \
    } while (0)
    LBC_DISPATCH_ACT(a.act_bf16, LBC_K, rows);
#undef LBC_K
    return lbc_check_launch("maxpool_relu_bwd_reduce");
}
