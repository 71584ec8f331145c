// Device-resident LMDB dataset (bird_view/utils/datasets/resident.py ResidentLoader): what DeviceLoader._fill does per sample on the
// host -- look the frame up, copy its bytes into staging, derive the waypoints -- as kernels over a whole batch of frames that already
// live in HBM.  The host only draws: one record of four int32 per sample, (frame index, delta_angle in degrees, dx, dy).
//   gather_crop        dst[b * reps + r] = the window [y0, y0 + H) x [x0, x0 + W) of src frame idx[b] (the fixed bird-view crop of
//                      reference image_lmdb.py:150-163 through an index; with the whole frame as the window, the plain row gather of the
//                      camera frames).  16 bytes per lane where row bytes, row offset, source row pitch and both bases are multiples of
//                      16 (the stored map: 192 * 7 = 1,344-byte rows at a 448-byte offset, 2,240-byte pitch), a byte per lane otherwise.
//   gather_warp_crop   the indexed form of data.hip's warp_crop_u8_k (reference birdview_lmdb.py:103-125): the frame is draw.idx, the
//                      inverted matrix is table[delta_angle + A] -- one entry per integer angle, computed on the host by the same
//                      warp_params() the host loader uses, so no device cos / sin feeds the fixed-point coordinates -- and the window
//                      origin follows (dx, dy).  The pixel is lbc_warp_pixel_u8, the function warp_crop_u8_k calls.
//   targets            ImageDataset.raw()'s waypoints and speed, one lane per sample, from the measurement table (x, y, heading, speed,
//                      cmd as f32, one row per stored frame, episodes contiguous): the future positions are rows row + k * gap.
//   gather_rows        dst row b * reps + r = src row draws[b * stride] for f32 rows: the cached waypoints of the frozen teacher
//                      (--cache-teacher, 50 floats per frame) through the record (stride 4) or a dense index vector (stride 1).
// Every offset is 64-bit: 2,996 stored maps pass 2^31 bytes.
#include "lbc_common.hpp"
#include "lbc_kernels.hpp"
#include "lbc_warp.hpp"

namespace {

// Window copy through an index, 16 bytes per lane, U chunks in flight per lane.  Workgroup (x, y): chunks [x * 256 * U, ...) of the
// output frames y, y + gridDim.y, ...; a frame's window is H rows of cpr chunks, the source row pitch is spr chunks, x0c the window's
// column offset in chunks.
template <int U>
__global__ __launch_bounds__(256) void gather_crop_vec_k(const uint4* __restrict__ src, const int* __restrict__ idx, long long frames, int reps,
                                                         long long frame_chunks, int spr, int y0, int x0c, int H, int cpr, uint4* __restrict__ dst)
{
    const unsigned chunks = (unsigned)H * (unsigned)cpr;                       // (< 2^30: checked by the launcher; 32-bit divisions below)
    const unsigned c0 = blockIdx.x * (256u * U) + threadIdx.x;
    for (long long r = blockIdx.y; r < frames; r += gridDim.y) {
        const uint4* s = src + (long long)idx[r / reps] * frame_chunks + (long long)y0 * spr + x0c;
        uint4* d = dst + r * (long long)chunks;
        if ((blockIdx.x + 1) * (256u * U) <= chunks) {                         // a whole span: U loads in flight, then U stores
            uint4 v[U];
#pragma unroll
            for (int k = 0; k < U; ++k) {
                const unsigned c = c0 + k * 256u, y = c / (unsigned)cpr;
                v[k] = s[(long long)y * spr + (c - y * (unsigned)cpr)];
            }
#pragma unroll
            for (int k = 0; k < U; ++k) d[c0 + k * 256u] = v[k];
        } else {                                                               // the window's last span
            for (unsigned c = c0; c < chunks; c += 256u) {
                const unsigned y = c / (unsigned)cpr;
                d[c] = s[(long long)y * spr + (c - y * (unsigned)cpr)];
            }
        }
    }
}

// the same copy a byte per lane: rows or offsets that are no multiple of 16 bytes
__global__ __launch_bounds__(256) void gather_crop_byte_k(const unsigned char* __restrict__ src, const int* __restrict__ idx, long long frames, int reps,
                                                          int SH, int SW, int C, int y0, int x0, int H, int W, unsigned char* __restrict__ dst)
{
    const long long row_bytes = (long long)W * C;
    const long long total = frames * H * row_bytes;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const long long row = i / row_bytes;
        const long long b = i - row * row_bytes;
        const long long r = row / H;
        const long long y = row - r * H;
        dst[i] = src[(((long long)idx[r / reps] * SH + (y0 + y)) * SW + x0) * C + b];
    }
}

struct Draw { int idx, delta_angle, dx, dy; };      // one sample's record, as the host uploads it

__global__ __launch_bounds__(256) void gather_warp_crop_u8_k(const unsigned char* __restrict__ src, const Draw* __restrict__ draws,
                                                             const WarpParams* __restrict__ table, int A, long long frames, int reps, int SH, int SW,
                                                             int C, int H, int W, int oy, int ox, unsigned char* __restrict__ dst)
{
    const long long total = frames * H * W;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const long long r = i / ((long long)H * W);
        const int pix = (int)(i - r * H * W);
        const Draw dr = draws[r / reps];
        const WarpParams& p = table[dr.delta_angle + A];
        const int y = dr.dy + oy + pix / W, x = dr.dx + ox + pix % W;
        lbc_warp_pixel_u8(src + (long long)dr.idx * SH * SW * C, dst + i * C, p.im, y, x, SH, SW, C);
    }
}

// ImageDataset.raw() (reference image_lmdb.py:143-163, birdview_lmdb.py:127-141) in its own precisions: (x - ox) * 5 in f32 (numpy keeps
// f32 there), the angle = the stored f32 heading + the jitter in double, the rotation and every offset in double, one cast at the end
__global__ __launch_bounds__(256) void targets_k(const float* __restrict__ table, const int* __restrict__ row_of_sample, const Draw* __restrict__ draws,
                                                 int B, int reps, int gap, int n_step, int img_size, int crop_size, float* __restrict__ loc,
                                                 float* __restrict__ speed)
{
    const int b = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (b >= B) return;
    const Draw dr = draws[b];
    const long long row = row_of_sample[dr.idx];
    const float* m = table + row * 5;
    const float ox = m[0], oy = m[1];
    const double angle = (double)m[2] + (double)dr.delta_angle * (3.14159265358979323846 / 180.0);
    const double c = cos(angle), s = sin(angle);
    const float sp = m[3];
    for (int r = 0; r < reps; ++r) speed[(long long)b * reps + r] = sp;
    for (int k = 0; k < n_step; ++k) {
        const float* f = table + (row + (long long)(k + 1) * gap) * 5;
        const float pdx = (f[0] - ox) * 5.f, pdy = (f[1] - oy) * 5.f;        // PIXELS_PER_METER
        // world_to_pixel: the rotated offset, mirrored, + offset (-80, 160); the caller names the pair (pixel_y, pixel_x)
        const double py = 320.0 - ((double)pdx * c + (double)pdy * s) + -80.0;
        const double px = (-(double)pdx * s + (double)pdy * c) + 160.0;
        const double lx = px - (double)((img_size - crop_size) / 2) - (double)dr.dx;
        const double ly = (double)crop_size - ((double)img_size - py) + 70.0 - (double)dr.dy;
        for (int r = 0; r < reps; ++r) {
            float* o = loc + (((long long)b * reps + r) * n_step + k) * 2;
            o[0] = (float)lx;
            o[1] = (float)ly;
        }
    }
}

// Row copy through an index: word i of output row (b * reps + r) = word i of source row draws[b * stride], rows of W words of type T
// (uint2: the cached teacher rows are 200 bytes, which 8 divides and 16 does not; unsigned: odd rows and bases that are not 8-byte
// aligned).  Integer words, so a NaN's payload and the sign of a zero pass through untouched.
template <typename T>
__global__ __launch_bounds__(256) void gather_rows_k(const T* __restrict__ src, const int* __restrict__ draws, int stride, long long rows, int reps,
                                                     int W, T* __restrict__ dst)
{
    const long long total = rows * W;
    const long long step = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += step) {
        const long long row = i / W;
        const int j = (int)(i - row * W);
        dst[i] = src[(long long)draws[(row / reps) * stride] * W + j];
    }
}

int grid_1d(long long total)
{
    long long b = (total + 255) / 256;
    if (b > 8192) b = 8192;
    return (int)(b < 1 ? 1 : b);
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

int lbc_dataset_gather_crop_launch(const unsigned char* src, const int* idx, int B, int reps, int SH, int SW, int C, int y0, int x0, int H, int W,
                                   unsigned char* dst, hipStream_t s)
{
    LBC_REQUIRE(src && idx && dst, "dataset_gather_crop_u8: null argument");
    LBC_REQUIRE(B >= 1 && reps >= 1, "dataset_gather_crop_u8: B = %d, reps = %d, both must be positive", B, reps);
    LBC_REQUIRE(C > 0 && H > 0 && W > 0 && y0 >= 0 && x0 >= 0 && y0 + H <= SH && x0 + W <= SW,
                "dataset_gather_crop_u8: window %d x %d at (%d, %d) outside the %d x %d source", H, W, y0, x0, SH, SW);
    const long long frames = (long long)B * reps;
    const long long row_bytes = (long long)W * C, pitch = (long long)SW * C, off = (long long)x0 * C;
    LbcProfScope prof("dataset_gather_crop_u8", 0.0, 2.0 * (double)frames * H * (double)row_bytes, s);
    if (row_bytes % 16 == 0 && pitch % 16 == 0 && off % 16 == 0 && ((long long)SH * pitch) % 16 == 0 && aligned16(src) && aligned16(dst)) {
        const int cpr = (int)(row_bytes / 16), spr = (int)(pitch / 16);
        const long long chunks = (long long)H * cpr;
        LBC_REQUIRE(chunks < (1LL << 30), "dataset_gather_crop_u8: a window of %lld 16-byte words", chunks);
        // 16 KB per workgroup once that still yields a thousand workgroups, 4 KB below (as replay.hip's row copy)
        const bool wide = frames * chunks >= 1024LL * 1024;
        const long long per = wide ? 1024 : 256;
        const dim3 grid((unsigned)((chunks + per - 1) / per), (unsigned)(frames < 65535 ? frames : 65535));
        const uint4* s16 = reinterpret_cast<const uint4*>(src);
        uint4* d16 = reinterpret_cast<uint4*>(dst);
        if (wide)
            hipLaunchKernelGGL(gather_crop_vec_k<4>, grid, dim3(256), 0, s, s16, idx, frames, reps, (long long)SH * spr, spr, y0, (int)(off / 16), H, cpr, d16);
        else
            hipLaunchKernelGGL(gather_crop_vec_k<1>, grid, dim3(256), 0, s, s16, idx, frames, reps, (long long)SH * spr, spr, y0, (int)(off / 16), H, cpr, d16);
    } else {
        hipLaunchKernelGGL(gather_crop_byte_k, dim3((unsigned)grid_1d(frames * H * row_bytes)), dim3(256), 0, s, src, idx, frames, reps, SH, SW, C, y0, x0,
                           H, W, dst);
    }
    return lbc_check_launch("dataset_gather_crop_u8");
}

int lbc_dataset_gather_warp_crop_launch(const unsigned char* src, const int* draws, const WarpParams* table, int A, int B, int reps, int SH, int SW, int C,
                                        int H, int W, unsigned char* dst, hipStream_t s)
{
    LBC_REQUIRE(src && draws && table && dst, "dataset_gather_warp_crop_u8: null argument");
    LBC_REQUIRE(A >= 0 && B >= 1 && reps >= 1 && SH > 1 && SW > 1 && C > 0 && H > 0 && W > 0, "dataset_gather_warp_crop_u8: bad arguments");
    const long long frames = (long long)B * reps;
    LbcProfScope prof("dataset_gather_warp_crop_u8", 0.0, 5.0 * (double)frames * H * (double)W * C, s);
    // the window origin of warp_params(): rows dy + (260 - H / 2) - H / 2, columns dx + 160 - W / 2 (164 - 96 and 160 - 96 at 192 x 192)
    hipLaunchKernelGGL(gather_warp_crop_u8_k, dim3((unsigned)grid_1d(frames * H * W)), dim3(256), 0, s, src, reinterpret_cast<const Draw*>(draws), table, A,
                       frames, reps, SH, SW, C, H, W, 260 - H / 2 - H / 2, 160 - W / 2, dst);
    return lbc_check_launch("dataset_gather_warp_crop_u8");
}

int lbc_dataset_targets_launch(const float* table, const int* row_of_sample, const int* draws, int B, int reps, int gap, int n_step, int img_size,
                               int crop_size, float* loc, float* speed, hipStream_t s)
{
    LBC_REQUIRE(table && row_of_sample && draws && loc && speed, "dataset_targets: null argument");
    LBC_REQUIRE(B >= 1 && reps >= 1 && gap >= 1 && n_step >= 1 && img_size >= crop_size && crop_size > 0,
                "dataset_targets: B = %d, reps = %d, gap = %d, n_step = %d, img_size = %d, crop_size = %d", B, reps, gap, n_step, img_size, crop_size);
    hipLaunchKernelGGL(targets_k, dim3((unsigned)lbc_cdiv(B, 256)), dim3(256), 0, s, table, row_of_sample, reinterpret_cast<const Draw*>(draws), B, reps, gap,
                       n_step, img_size, crop_size, loc, speed);
    return lbc_check_launch("dataset_targets");
}

int lbc_dataset_gather_rows_launch(const float* src, const int* draws, int stride, int B, int reps, int R, float* dst, hipStream_t s)
{
    LBC_REQUIRE(src && draws && dst, "dataset_gather_rows_f32: null argument");
    LBC_REQUIRE(B >= 1 && reps >= 1 && R >= 1 && stride >= 1, "dataset_gather_rows_f32: B = %d, reps = %d, R = %d, stride = %d, all must be positive", B,
                reps, R, stride);
    const long long rows = (long long)B * reps;
    LbcProfScope prof("dataset_gather_rows_f32", 0.0, 8.0 * (double)rows * R, s);
    const bool pairs = R % 2 == 0 && (reinterpret_cast<uintptr_t>(src) & 7) == 0 && (reinterpret_cast<uintptr_t>(dst) & 7) == 0;
    if (pairs)
        hipLaunchKernelGGL(gather_rows_k<uint2>, dim3((unsigned)grid_1d(rows * (R / 2))), dim3(256), 0, s, reinterpret_cast<const uint2*>(src), draws, stride,
                           rows, reps, R / 2, reinterpret_cast<uint2*>(dst));
    else
        hipLaunchKernelGGL(gather_rows_k<unsigned>, dim3((unsigned)grid_1d(rows * R)), dim3(256), 0, s, reinterpret_cast<const unsigned*>(src), draws, stride,
                           rows, reps, R, reinterpret_cast<unsigned*>(dst));
    return lbc_check_launch("dataset_gather_rows_f32");
}
