// 16.16 fixed-point R'G'B' -> Y'CbCr coefficients of jh_blit_yuv (include/jello_hip.h).
// kYuvMatrix[jh_yuv_matrix][jh_yuv_range] = {Y row, Cb row, Cr row}: round-half-even(exact * 2^16) of the BT.601 / BT.709
// coefficients scaled by 219/255 (luma) and 224/255 (chroma) in limited range, the green coefficient adjusted so that
// the Y row sums to rne(scale * 2^16) and each chroma row to 0.  kYuvOffset[jh_yuv_range] is the luma offset.
// Generated -- do not edit:
//     python tools/gen_yuv_table.py
#pragma once
static const int kYuvMatrix[2][2][9] = {
    {
        {16829, 33039, 6416,  -9714, -19070, 28784,  28784, -24103, -4681},  // BT601 LIMITED
        {19595, 38470, 7471,  -11058, -21710, 32768,  32768, -27439, -5329},  // BT601 FULL
    },
    {
        {11966, 40254, 4064,  -6596, -22188, 28784,  28784, -26145, -2639},  // BT709 LIMITED
        {13933, 46871, 4732,  -7509, -25259, 32768,  32768, -29763, -3005},  // BT709 FULL
    },
};
static const int kYuvOffset[2] = {16, 0};
