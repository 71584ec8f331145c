// One destination pixel of the bird-view rotation + crop (data.hip warp_crop_u8_k, dataset.hip gather_warp_crop_u8_k): OpenCV's 8-bit
// bilinear cv2.warpAffine restated (imgwarp.cpp, remap with INTER_BITS = 5) -- source coordinates in 1/1024 fixed point from the INVERTED
// matrix (rounded half to even like cvRound, + 16, >> 5 -> 1/32 pixel), a 32 x 32 table of 15-bit weights whose four entries sum to
// 32768, (sum + 16384) >> 15, zero outside the image (BORDER_CONSTANT).  Both kernels call this one function, so that a frame warped
// through an index is bit for bit the frame warped in place.
#pragma once
#include "lbc_common.hpp"

// frame: the source image [SH][SW][C]; im: the inverted matrix (iM0, iM1, b1, iM3, iM4, b2); (y, x): the pixel in the warped image;
// d: its C output bytes
__device__ __forceinline__ void lbc_warp_pixel_u8(const unsigned char* __restrict__ frame, unsigned char* __restrict__ d, const double* im, int y, int x,
                                                  int SH, int SW, int C)
{
    const int adelta = (int)rint(im[0] * x * 1024.0), bdelta = (int)rint(im[3] * x * 1024.0);
    const int X0 = (int)rint((im[1] * y + im[2]) * 1024.0) + 16, Y0 = (int)rint((im[4] * y + im[5]) * 1024.0) + 16;
    const int X = (X0 + adelta) >> 5, Y = (Y0 + bdelta) >> 5;
    const int sx = X >> 5, sy = Y >> 5, fx = X & 31, fy = Y & 31;
    // the weights of table entry (fy, fx)
    const float ax = (float)fx * (1.f / 32.f), ay = (float)fy * (1.f / 32.f);
    const float wf[4] = {(1.f - ay) * (1.f - ax), (1.f - ay) * ax, ay * (1.f - ax), ay * ax};
    // (bilinear weights are products of two multiples of 1/32: every w[k] is an exact multiple of 32 and the four sum to 32768
    //  exactly -- OpenCV's fix-up of the table sum can never fire for INTER_LINEAR, it is not restated)
    int w[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) w[k] = (int)rintf(wf[k] * 32768.f);
    const bool in00 = (unsigned)sy < (unsigned)SH && (unsigned)sx < (unsigned)SW, in01 = (unsigned)sy < (unsigned)SH && (unsigned)(sx + 1) < (unsigned)SW;
    const bool in10 = (unsigned)(sy + 1) < (unsigned)SH && (unsigned)sx < (unsigned)SW, in11 = (unsigned)(sy + 1) < (unsigned)SH && (unsigned)(sx + 1) < (unsigned)SW;
    const unsigned char* s0 = frame + ((long long)sy * SW + sx) * C;
    for (int c = 0; c < C; ++c) {
        const int v00 = in00 ? s0[c] : 0, v01 = in01 ? s0[C + c] : 0, v10 = in10 ? s0[(long long)SW * C + c] : 0, v11 = in11 ? s0[(long long)SW * C + C + c] : 0;
        const int v = (v00 * w[0] + v01 * w[1] + v10 * w[2] + v11 * w[3] + (1 << 14)) >> 15;
        d[c] = (unsigned char)(v < 0 ? 0 : (v > 255 ? 255 : v));
    }
}
