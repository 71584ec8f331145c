// Training visuals for gfx950 (include/lbc_hip.h lbc_visuals_render): one launch draws the grid of waypoint panels the reference's
// _log_visuals builds on the host (training/train_image_phase0.py:91-147, train_image_phase1.py:72-128, train_birdview.py:57-99) into
// one uint8 HWC image in device memory.  Nothing is read back: the caller copies the image when it wants a file.
//
// Shape: a 1-D grid of workgroups of 256 threads; a workgroup owns 4,096 consecutive pixels of the image in row-major order, a thread
// owns four consecutive pixels of them per iteration (four iterations, each one coalesced over the workgroup) and stores their twelve
// bytes with ONE 12-byte store (the image base is 4-byte aligned and 12 g is a multiple of 4 whatever the row length; only the last
// one to three pixels of an image whose pixel count is no multiple of four go out as bytes).  The kernel is a gather: every pixel is
// decided -- padding, black band, text, dot, frame byte, map colour -- and written exactly once, so there is no write race, no atomic
// and the same inputs give the same bytes on every run.
// Preamble of every workgroup, in LDS: (1) the rank of each of the <= 32 candidates by loss (thread t counts the candidates that come
// before candidate t: 32 compares) -> the sample of every panel slot, no second launch; (2) for the slots of the panel rows this
// workgroup's pixels touch: the twenty dot centres of the sample (ten on the map canvas, ten on the camera frame; a centre that is
// not drawn is a sentinel no pixel comes near) in double from the f32 inputs, and the two text lines with the loss formatted on the
// device.  The pixel loop then only compares integers.
// Why there is no scratch: nothing is indexed dynamically but LDS and global memory.  The colour table is walked by an unrolled loop
// (its entries become immediates), the base-10^9 limbs of the loss are five scalars behind unrolled loops, the strings are literals.
// Reads: rgb [N][H][W][3] u8 or [N][3][H][W] f32, birdview [N][BH][BW][7] u8 or [N][7][BH][BW] f32 (nullable), pred / teacher
// [N][5][2] or [N][4][5][2] f32, command [N][4], loss [N] -- all at sample indices below min(N, size) -- and the 665 bytes of the
// glyph table.  Writes: the rows x cols x 3 bytes of the image, every one of them, and nothing else.
#include "lbc_common.hpp"
#include "lbc_hip.h"
#include "lbc_kernels.hpp"
#include <math.h>
#include <stddef.h>

namespace {

constexpr int kThreads = 256, kPix = 4, kIter = 4, kBlockPixels = kThreads * kPix * kIter;
constexpr int kMaxShow = 32;         // panels (lbc_visuals_desc.size)
constexpr int kDots = 20;            // per sample: 0..9 on the canvas, 10..19 on the frame; the second five of each are RED
constexpr int kTextMax = 56;         // "Loss: -" + 41 digits (FLT_MAX x 100) + ".00" = 51 characters
constexpr int kPad = 2;              // black pixels around and between panels
constexpr int kGlyphW = 5, kGlyphH = 7, kAdvance = 6, kLinePitch = 19;      // line k = 1, 2 occupies canvas rows 19 k - 6 .. 19 k
constexpr int kNone = 1 << 30;       // the centre of a dot that is not drawn: no pixel coordinate comes within 2 of it
constexpr unsigned kWhite = 0xFFFFFFu, kBlue = 0xFF0000u, kRed = 0x0000FFu;       // packed R | G << 8 | B << 16
constexpr unsigned rgb_of(unsigned r, unsigned g, unsigned b) { return r | (g << 8) | (b << 16); }
// the reference's bird_view/utils/carla_utils.py BACKGROUND and COLORS (road, lane, red / yellow / green light, vehicle, pedestrian)
constexpr unsigned kBackground = rgb_of(0, 47, 0);
constexpr unsigned color_of(int i)
{
    return i == 0 ? rgb_of(102, 102, 102) : i == 1 ? rgb_of(253, 253, 17) : i == 2 ? rgb_of(204, 6, 5) : i == 3 ? rgb_of(250, 210, 1)
         : i == 4 ? rgb_of(39, 232, 51) : i == 5 ? rgb_of(0, 0, 142) : rgb_of(220, 20, 60);
}

struct VisArgs {
    const void* rgb; const void* bv; const float* pred; const float* teach; const float* cmd; const float* loss;
    const unsigned char* font; unsigned char* out;
    int mode, M, sort, ncols, H, W, BH, BW, rgb_f32, bv_f32;
    int PH, PW, FW, top;             // panel rows / columns, columns of the frame part (0 in mode 2), first panel row of the frame
    unsigned cellh, cellw, cols, total;      // panel + padding, image columns, image pixels
    double w, h, f, world_y, fixed_offset, ppm, crop;
};

struct __attribute__((aligned(4))) Bytes12 { unsigned a, b, c; };

// the first non-zero entry of a command row, -1 if there is none
__device__ __forceinline__ int command_of(const VisArgs& a, int s)
{
    const float* cm = a.cmd + (size_t)s * 4;
    int c = -1;
#pragma unroll
    for (int k = 3; k >= 0; --k) c = (cm[k] != 0.f) ? k : c;
    return c;
}

// centre of dot d of sample s (command c) -> LDS; see the table in include/lbc_hip.h
__device__ __forceinline__ void dot_centre(const VisArgs& a, int s, int c, int d, int* out)
{
    const int frame = d / 10, second = (d % 10) / 5, t = d % 5;
    const bool all = a.mode == 1;                                   // (N,4,5,2): the commanded branch
    const size_t o = all ? (((size_t)s * 4 + (c < 0 ? 0 : c)) * 5 + t) * 2 : ((size_t)s * 5 + t) * 2;
    double x = 0.0, y = 0.0;
    bool have = false;
    if (!all || c >= 0) {
        const double tx = (double)a.teach[o], ty = (double)a.teach[o + 1];
        const double px = (double)a.pred[o], py = (double)a.pred[o + 1];
        if (!frame && !second) {                                    // teacher / ground truth on the map
            x = a.mode == 2 ? tx : (tx + 1.0) * a.crop / 2.0;
            y = a.mode == 2 ? ty : (ty + 1.0) * a.crop / 2.0;
            have = true;
        } else if (!frame && a.mode == 1) {                         // the student, unprojected (csrc/metrics.hip row_err, frame 0)
            const double lx = (px + 1.0) * a.w / 2.0, ly = (py + 1.0) * a.h / 2.0;
            const double xt = (lx - a.w / 2.0) / a.f, yt = (ly - a.h / 2.0) / a.f;
            const double wz = a.world_y / yt, wx = wz * xt;
            x = wx * a.ppm + a.crop / 2.0;
            y = a.crop - wz * a.ppm + a.fixed_offset * a.ppm;
            have = true;
        } else if (!frame && a.mode == 2) {                         // the privileged agent's prediction on the map
            x = (px + 1.0) * a.crop / 2.0;
            y = (py + 1.0) * a.crop / 2.0;
            have = true;
        } else if (frame && !second && a.mode == 0) {               // the teacher, projected into the camera (train_image_phase0.py:54-79)
            const double mx = (tx + 1.0) * a.crop / 2.0, my = (ty + 1.0) * a.crop / 2.0;
            const double X = (mx - a.crop / 2.0) / a.ppm, Z = (a.crop - my) / a.ppm + a.fixed_offset;
            const double u = a.f * X / Z + a.w / 2.0, v = a.f * a.world_y / Z + a.h / 2.0;
            x = u < 0.0 ? 0.0 : (u > a.w ? a.w : u);                // np.clip: a NaN stays a NaN
            y = v < 0.0 ? 0.0 : (v > a.h ? a.h : v);
            have = true;
        } else if (frame && second && a.mode != 2) {                // the student in the camera frame
            x = (px + 1.0) * a.w / 2.0;
            y = (py + 1.0) * a.h / 2.0;
            have = true;
        }
    }
    const bool ok = have && __builtin_isfinite(x) && __builtin_isfinite(y) && fabs(x) < 1073741824.0 && fabs(y) < 1073741824.0;
    out[0] = ok ? (int)x : kNone;                                   // (int) truncates toward zero
    out[1] = ok ? (int)y : kNone;
}

__device__ __forceinline__ int put(unsigned char* line, int n, const char* s)
{
    for (int i = 0; s[i]; ++i) line[n++] = (unsigned char)s[i];
    return n;
}

// "Command: <name>" and "Loss: <%.2f>" of sample s -> LDS; -> the two lengths
__device__ __forceinline__ void format_text(const VisArgs& a, int s, int c, unsigned char* l1, unsigned char* l2, int* len)
{
    int n = put(l1, 0, "Command: ");
    len[0] = put(l1, n, c == 0 ? "LEFT" : c == 1 ? "RIGHT" : c == 2 ? "STRAIGHT" : c == 3 ? "FOLLOW" : "???");
    n = put(l2, 0, "Loss: ");
    const double v = (double)a.loss[s];
    if (v != v) { len[1] = put(l2, n, "nan"); return; }
    if (!__builtin_isfinite(v)) { len[1] = put(l2, n, v < 0.0 ? "-inf" : "inf"); return; }
    if (__builtin_signbit(v)) l2[n++] = '-';
    // hundredths, rounded half to even: an f32 times 100 is exact in double (24 + 7 bits), so this is the decimal rounding of the
    // value itself -- what '%.2f' prints
    double q = rint(fabs(v) * 100.0);
    int e = 0;
    while (q >= 9007199254740992.0) { q *= 0.5; ++e; }             // q = m 2^e, m < 2^53: exact (q has at most 31 significant bits)
    unsigned long long m = (unsigned long long)q;
    unsigned L[5];                                                  // base 10^9, least significant first; FLT_MAX x 100 < 10^41
    L[0] = (unsigned)(m % 1000000000ull); m /= 1000000000ull;
    L[1] = (unsigned)(m % 1000000000ull);
    L[2] = (unsigned)(m / 1000000000ull);
    L[3] = 0; L[4] = 0;
    for (int i = 0; i < e; ++i) {
        unsigned carry = 0;
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            unsigned t = L[k] * 2u + carry;
            carry = t >= 1000000000u ? 1u : 0u;
            L[k] = t - carry * 1000000000u;
        }
    }
    bool started = false;
#pragma unroll
    for (int k = 4; k >= 0; --k) {
        unsigned r = L[k], div = 100000000u;
#pragma unroll
        for (int j = 8; j >= 0; --j) {
            const unsigned dgt = r / div;
            r -= dgt * div;
            div /= 10u;
            const int after = k * 9 + j;                            // digits behind this one
            if (after == 1) l2[n++] = '.';
            started = started || dgt != 0u || after <= 2;           // at least one digit in front of the point
            if (started) l2[n++] = (unsigned char)('0' + dgt);
        }
    }
    len[1] = n;
}

__device__ __forceinline__ bool hits(int px, int py, const int* centre)
{
    return (unsigned)(px - centre[0] + 2) <= 4u && (unsigned)(py - centre[1] + 2) <= 4u;
}

// the packed colour of image pixel (r, c)
__device__ __forceinline__ unsigned pixel(const VisArgs& a, unsigned r, unsigned c, const int* s_sample, int (*s_dot)[kDots][2],
                                          unsigned char (*s_text)[2][kTextMax], int (*s_len)[2])
{
    if (r < (unsigned)kPad || c < (unsigned)kPad) return 0u;
    const unsigned rr = r - kPad, cc = c - kPad;
    const unsigned pr = rr / a.cellh, y = rr - pr * a.cellh;
    const unsigned pc = cc / a.cellw, x = cc - pc * a.cellw;
    if (y >= (unsigned)a.PH || x >= (unsigned)a.PW) return 0u;       // the padding below and right of a panel
    const unsigned long long slot = (unsigned long long)pr * (unsigned)a.ncols + pc;
    if (slot >= (unsigned long long)a.M) return 0u;                  // an unused slot of the last row
    const int s = s_sample[slot];
    if (x >= (unsigned)a.FW) {
        // ---- the map canvas: text over dots over the coloured bird-view
        const int cx = (int)x - a.FW, cy = (int)y;
        const int line = (cy >= kLinePitch - 6 && cy <= kLinePitch) ? 0 : (cy >= 2 * kLinePitch - 6 && cy <= 2 * kLinePitch) ? 1 : -1;
        if (line >= 0) {
            const int gy = cy - ((line + 1) * kLinePitch - 6), ci = cx / kAdvance, gx = cx - ci * kAdvance;
            if (gx < kGlyphW && ci < s_len[s][line]) {
                const int ch = s_text[s][line][ci];
                if ((a.font[(ch - 32) * kGlyphH + gy] >> (kGlyphW - 1 - gx)) & 1) return kWhite;
            }
        }
        for (int d = 9; d >= 0; --d)                                  // a later dot covers an earlier one
            if (hits(cx, cy, s_dot[s][d])) return d >= 5 ? kRed : kBlue;
        unsigned col = kBackground;
        if (a.bv) {
            if (a.bv_f32) {
                const float* p = static_cast<const float*>(a.bv) + ((size_t)s * 7 * a.BH + cy) * a.BW + cx;
                const size_t plane = (size_t)a.BH * a.BW;
#pragma unroll
                for (int i = 0; i < 7; ++i) col = p[i * plane] > 0.f ? color_of(i) : col;
            } else {
                const unsigned char* p = static_cast<const unsigned char*>(a.bv) + (((size_t)s * a.BH + cy) * a.BW + cx) * 7;
#pragma unroll
                for (int i = 0; i < 7; ++i) col = p[i] > 0 ? color_of(i) : col;
            }
        }
        return col;
    }
    // ---- the camera frame between two black bands
    const int fx = (int)x, fy = (int)y - a.top;
    if (fy < 0 || fy >= a.H) return 0u;
    for (int d = 19; d >= 10; --d)
        if (hits(fx, fy, s_dot[s][d])) return d >= 15 ? kRed : kBlue;
    unsigned ch[3];
    if (a.rgb_f32) {
        const float* p = static_cast<const float*>(a.rgb) + ((size_t)s * 3 * a.H + fy) * a.W + fx;
        const size_t plane = (size_t)a.H * a.W;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const float v = p[i * plane] * 255.0f;                    // np.uint8(x * 255): f32 product, truncated
            ch[i] = v >= 255.0f ? 255u : (v > 0.f ? (unsigned)(int)v : 0u);
        }
    } else {
        const unsigned char* p = static_cast<const unsigned char*>(a.rgb) + (((size_t)s * a.H + fy) * a.W + fx) * 3;
#pragma unroll
        for (int i = 0; i < 3; ++i) ch[i] = p[i];
    }
    return ch[0] | (ch[1] << 8) | (ch[2] << 16);
}

__global__ __launch_bounds__(kThreads) void visuals_render_k(VisArgs a)
{
    __shared__ int s_sample[kMaxShow];                       // panel slot -> sample
    __shared__ int s_dot[kMaxShow][kDots][2];                // by sample
    __shared__ unsigned char s_text[kMaxShow][2][kTextMax];
    __shared__ int s_len[kMaxShow][2];
    const int tid = threadIdx.x;

    // (1) slot of every candidate: rank by loss, descending, NaN first, ties by index -- or the identity
    if (tid < a.M) {
        int rank = tid;
        if (a.sort) {
            const float mine = a.loss[tid];
            const bool mine_nan = mine != mine;
            rank = 0;
            for (int j = 0; j < a.M; ++j) {
                const float o = a.loss[j];
                const bool o_nan = o != o;
                const bool greater = (o_nan && !mine_nan) || o > mine;
                const bool equal = (o_nan && mine_nan) || o == mine;
                rank += (greater || (equal && j < tid)) ? 1 : 0;
            }
        }
        s_sample[rank] = tid;
    }
    __syncthreads();

    // (2) the slots of the panel rows this workgroup's pixels touch
    const unsigned p_first = blockIdx.x * (unsigned)kBlockPixels;
    const unsigned p_end = a.total - p_first < (unsigned)kBlockPixels ? a.total : p_first + kBlockPixels;
    const unsigned r_first = p_first / a.cols, r_last = (p_end - 1) / a.cols;
    const unsigned pr_first = r_first < (unsigned)kPad ? 0u : (r_first - kPad) / a.cellh;
    const unsigned pr_last = r_last < (unsigned)kPad ? 0u : (r_last - kPad) / a.cellh;
    const unsigned long long k_lo = (unsigned long long)pr_first * (unsigned)a.ncols, k_hi = ((unsigned long long)pr_last + 1) * (unsigned)a.ncols;
    const int k0 = k_lo < (unsigned long long)a.M ? (int)k_lo : a.M, k1 = k_hi < (unsigned long long)a.M ? (int)k_hi : a.M;
    for (int item = tid; item < (k1 - k0) * kDots; item += kThreads) {
        const int s = s_sample[k0 + item / kDots], d = item % kDots;
        dot_centre(a, s, command_of(a, s), d, s_dot[s][d]);
    }
    for (int item = tid; item < k1 - k0; item += kThreads) {
        const int s = s_sample[k0 + item];
        format_text(a, s, command_of(a, s), s_text[s][0], s_text[s][1], s_len[s]);
    }
    __syncthreads();

    // (3) the pixels
#pragma unroll 1
    for (int it = 0; it < kIter; ++it) {
        const unsigned p0 = p_first + ((unsigned)it * kThreads + tid) * kPix;
        if (p0 >= a.total) break;
        unsigned r = p0 / a.cols, c = p0 - r * a.cols;
        unsigned v[kPix];
#pragma unroll
        for (int i = 0; i < kPix; ++i) {
            v[i] = (p0 + i < a.total) ? pixel(a, r, c, s_sample, s_dot, s_text, s_len) : 0u;
            if (++c == a.cols) { c = 0; ++r; }
        }
        unsigned char* o = a.out + (size_t)p0 * 3;
        if (p0 + kPix <= a.total) {
            Bytes12 w;
            w.a = v[0] | (v[1] << 24);
            w.b = (v[1] >> 8) | (v[2] << 16);
            w.c = (v[2] >> 16) | (v[3] << 8);
            *reinterpret_cast<Bytes12*>(o) = w;
        } else {
            // the last one to three pixels of the image
            if (p0 + 0 < a.total) { o[0] = (unsigned char)v[0]; o[1] = (unsigned char)(v[0] >> 8); o[2] = (unsigned char)(v[0] >> 16); }
            if (p0 + 1 < a.total) { o[3] = (unsigned char)v[1]; o[4] = (unsigned char)(v[1] >> 8); o[5] = (unsigned char)(v[1] >> 16); }
            if (p0 + 2 < a.total) { o[6] = (unsigned char)v[2]; o[7] = (unsigned char)(v[2] >> 8); o[8] = (unsigned char)(v[2] >> 16); }
        }
    }
}

// the descriptor's own checks (shared by the shape query and the launch) -> panel and image extents
int check_desc(const lbc_visuals_desc* d, const char* who, int* PH, int* PW, long long* rows, long long* cols)
{
    LBC_REQUIRE(d, "%s: null descriptor", who);
    LBC_REQUIRE(d->struct_size == sizeof(lbc_visuals_desc),
                "%s: lbc_visuals_desc.struct_size is %u, this library (ABI %d) accepts %zu -- initialise the descriptor with LBC_VISUALS_DESC_INIT",
                who, d->struct_size, LBC_HIP_ABI_VERSION, sizeof(lbc_visuals_desc));
    LBC_REQUIRE(d->mode >= 0 && d->mode <= 2, "%s: mode = %d, must be 0 (phase 0), 1 (phase 1 / 2) or 2 (bird-view)", who, d->mode);
    LBC_REQUIRE(d->size >= 1 && d->size <= kMaxShow, "%s: size = %d outside 1..%d", who, d->size, kMaxShow);
    LBC_REQUIRE(d->ncols >= 1, "%s: ncols = %d, must be at least 1", who, d->ncols);
    LBC_REQUIRE(d->N >= 1, "%s: N = %d, must be at least 1", who, d->N);
    LBC_REQUIRE(d->BH >= 1 && d->BW >= 1 && d->BH <= 16384 && d->BW <= 16384, "%s: canvas %d x %d outside 1..16384", who, d->BH, d->BW);
    if (d->mode != 2)
        LBC_REQUIRE(d->H >= 1 && d->W >= 1 && d->W <= 16384 && d->H <= d->BH, "%s: frame %d x %d: both at least 1, W <= 16384, H <= BH = %d", who,
                    d->H, d->W, d->BH);
    *PH = d->BH;
    *PW = d->mode == 2 ? d->BW : d->W + d->BW;
    const int M = d->N < d->size ? d->N : d->size;
    *rows = kPad + (long long)lbc_cdiv(M, d->ncols) * (*PH + kPad);
    *cols = kPad + (long long)d->ncols * (*PW + kPad);
    LBC_REQUIRE(*rows * *cols < 2147483648ll / 4, "%s: an image of %lld x %lld pixels is too large (2^29 pixels at most)", who, *rows, *cols);
    return LBC_OK;
}

}  // namespace

int lbc_visuals_shape(const lbc_visuals_desc* d, int* rows, int* cols)
{
    int PH, PW;
    long long r, c;
    const int rc = check_desc(d, "visuals_image_shape", &PH, &PW, &r, &c);
    if (rc) return rc;
    LBC_REQUIRE(rows && cols, "visuals_image_shape: null result pointer");
    *rows = (int)r;
    *cols = (int)c;
    return LBC_OK;
}

int lbc_visuals_launch(const lbc_visuals_desc* d, const void* rgb, const void* birdview, const float* pred, const float* teacher,
                       const float* command_onehot, const float* loss, const unsigned char* font, unsigned char* out, hipStream_t s)
{
    int PH, PW;
    long long rows, cols;
    const int rc = check_desc(d, "visuals_render", &PH, &PW, &rows, &cols);
    if (rc) return rc;
    LBC_REQUIRE(d->mode == 2 || rgb, "visuals_render: null rgb in mode %d (only mode 2 draws no camera frame)", d->mode);
    LBC_REQUIRE(d->mode != 2 || birdview, "visuals_render: null birdview in mode 2 (modes 0 and 1 draw the background alone)");
    LBC_REQUIRE(pred && teacher && command_onehot && loss && font && out,
                "visuals_render: null argument (pred %p, teacher_or_target %p, command %p, loss %p, font %p, out %p)", (const void*)pred,
                (const void*)teacher, (const void*)command_onehot, (const void*)loss, (const void*)font, (const void*)out);
    LBC_REQUIRE((reinterpret_cast<uintptr_t>(out) & 3) == 0, "visuals_render: out (%p) must be 4-byte aligned", (const void*)out);
    VisArgs a;
    a.rgb = rgb; a.bv = birdview; a.pred = pred; a.teach = teacher; a.cmd = command_onehot; a.loss = loss; a.font = font; a.out = out;
    a.mode = d->mode; a.M = d->N < d->size ? d->N : d->size; a.sort = d->sort != 0; a.ncols = d->ncols;
    a.H = d->mode == 2 ? 0 : d->H; a.W = d->mode == 2 ? 0 : d->W; a.BH = d->BH; a.BW = d->BW;
    a.rgb_f32 = d->rgb_f32 != 0; a.bv_f32 = d->birdview_f32 != 0;
    a.PH = PH; a.PW = PW; a.FW = a.W; a.top = (a.BH - a.H) / 2;
    a.cellh = (unsigned)(PH + kPad); a.cellw = (unsigned)(PW + kPad); a.cols = (unsigned)cols; a.total = (unsigned)(rows * cols);
    const lbc_camera& c = d->camera;
    a.w = c.w; a.h = c.h; a.world_y = c.world_y; a.fixed_offset = c.fixed_offset; a.ppm = c.pixels_per_meter; a.crop = c.crop_size;
    a.f = (double)c.w / (2.0 * tan((double)c.fov * 3.14159265358979323846 / 360.0));      // the focal length, once, on the host
    // algorithmic bytes: the image written once; per panel the frame and the bird-view read once
    const double in_px = (double)a.M * ((double)a.H * a.W * (a.rgb_f32 ? 12.0 : 3.0) + (birdview ? (double)a.BH * a.BW * (a.bv_f32 ? 28.0 : 7.0) : 0.0));
    LbcProfScope prof("visuals", 0.0, 3.0 * (double)a.total + in_px, s);
    hipLaunchKernelGGL(visuals_render_k, dim3(lbc_cdiv(a.total, kBlockPixels)), dim3(kThreads), 0, s, a);
    return lbc_check_launch("visuals_render");
}
