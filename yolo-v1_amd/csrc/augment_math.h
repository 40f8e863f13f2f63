// Per-pixel colour arithmetic of the training augmentation, restating Pillow operation by operation so that the bytes
// agree: ImageEnhance.Brightness / ImageEnhance.Color (libImaging/Blend.c, the "L" conversion of Convert.c) and the
// RGB -> HSV -> RGB round trip with a shifted H byte (Convert.c rgb2hsv_row / hsv2rgb_row), for the Darknet recipe with scaled
// S and V bytes as well; and the address arithmetic of that recipe's window (edge replication) and mirror, so that a host
// probe can run the whole per-pixel pipeline of csrc/augment.hip.
// Every fp32 product that feeds a sum goes through the round-to-nearest intrinsics on the device (no FMA contraction);
// on the host (tests compile this header with a C++ compiler and compare it with Pillow) the same operations are plain
// IEEE arithmetic -- build such a probe with -ffp-contract=off.
#pragma once
#include <math.h>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif

#if defined(__HIPCC__)
#define AUG_FN __device__ __forceinline__
#define AUG_FMUL(a, b) __fmul_rn((a), (b))
#define AUG_FADD(a, b) __fadd_rn((a), (b))
#define AUG_FSUB(a, b) __fsub_rn((a), (b))
#define AUG_FDIV(a, b) __fdiv_rn((a), (b))
#define AUG_DMUL(a, b) __dmul_rn((a), (b))
#define AUG_DADD(a, b) __dadd_rn((a), (b))
#define AUG_DSUB(a, b) __dsub_rn((a), (b))
#define AUG_DDIV(a, b) __ddiv_rn((a), (b))
#else
#define AUG_FN static inline
#define AUG_FMUL(a, b) ((float)(a) * (float)(b))
#define AUG_FADD(a, b) ((float)(a) + (float)(b))
#define AUG_FSUB(a, b) ((float)(a) - (float)(b))
#define AUG_FDIV(a, b) ((float)(a) / (float)(b))
#define AUG_DMUL(a, b) ((double)(a) * (double)(b))
#define AUG_DADD(a, b) ((double)(a) + (double)(b))
#define AUG_DSUB(a, b) ((double)(a) - (double)(b))
#define AUG_DDIV(a, b) ((double)(a) / (double)(b))
#endif

namespace yolo_aug {

enum { OP_BRIGHTNESS = 0, OP_SATURATION = 1, OP_HUE = 2, OP_HSV = 4 };      // = YOLO_AUG_* (3 is not assigned)
enum { F_FLIP = 1, F_EDGE = 2 };                                            // = YOLO_AUG_F_*

// ImagingBlend: in1 + alpha * (in2 - in1), difference in int, the rest in fp32; inside [0, 1] the result is truncated
// without a clip, outside it is clipped first
AUG_FN int blend8(int in1, int in2, float alpha)
{
    const float t = AUG_FADD((float)in1, AUG_FMUL(alpha, (float)(in2 - in1)));
    if (alpha >= 0.0f && alpha <= 1.0f) return (int)t & 255;      // (UINT8) cast of an in-range value
    if (t <= 0.0f) return 0;
    if (t >= 255.0f) return 255;
    return (int)t;
}

AUG_FN void brightness(int &r, int &g, int &b, float fac)
{
    r = blend8(0, r, fac); g = blend8(0, g, fac); b = blend8(0, b, fac);
}

// ImageEnhance.Color: blend(convert("L").convert("RGB"), image, fac)
AUG_FN void saturation(int &r, int &g, int &b, float fac)
{
    const int L = (19595 * r + 38470 * g + 7471 * b + 0x8000) >> 16;
    r = blend8(L, r, fac); g = blend8(L, g, fac); b = blend8(L, b, fac);
}

AUG_FN int clip255(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// min(255, trunc(fl32(v) * fac)) for a byte v and a finite factor >= 0 (the comparison in fp32: the product may not fit an int)
AUG_FN int scale8(int v, float fac)
{
    const float t = AUG_FMUL((float)v, fac);
    return t >= 255.0f ? 255 : (int)t;
}

// convert("HSV"), H := (H + shift) mod 256, with `scale` also S := scale8(S, sfac) and V := scale8(V, vfac), convert("RGB")
// (one body for OP_HUE and OP_HSV: `scale` is uniform over the image, and two inlined copies made the kernel's colour loop larger)
AUG_FN void hsv_round_trip(int &r, int &g, int &b, int shift, bool scale, float sfac, float vfac)
{
    const int maxc = r > g ? (r > b ? r : b) : (g > b ? g : b);
    const int minc = r < g ? (r < b ? r : b) : (g < b ? g : b);
    int H = 0, S = 0, V = maxc;
    if (minc != maxc) {
        const float cr = (float)(maxc - minc);
        const float s = AUG_FDIV(cr, (float)maxc);
        const float rc = AUG_FDIV((float)(maxc - r), cr);
        const float gc = AUG_FDIV((float)(maxc - g), cr);
        const float bc = AUG_FDIV((float)(maxc - b), cr);
        float h;
        if (r == maxc) h = AUG_FSUB(bc, gc);
        else if (g == maxc) h = (float)AUG_DSUB(AUG_DADD(2.0, (double)rc), (double)bc);
        else h = (float)AUG_DSUB(AUG_DADD(4.0, (double)gc), (double)rc);
        h = (float)fmod(AUG_DADD(AUG_DDIV((double)h, 6.0), 1.0), 1.0);
        H = clip255((int)AUG_DMUL((double)h, 255.0));
        S = clip255((int)AUG_DMUL((double)s, 255.0));
    }
    H = (H + shift) & 255;          // two's complement: = ((H + shift) mod 256) for a negative shift too
    if (scale) {
        S = scale8(S, sfac);
        V = scale8(V, vfac);
    }
    if (S == 0) {
        r = g = b = V;
        return;
    }
    const double hf = AUG_DDIV(AUG_DMUL((double)(float)H, 6.0), 255.0);
    const double fl = floor(hf);
    const int i = (int)fl;
    const float fr = (float)AUG_DSUB(hf, (double)(float)i);
    const float fs = (float)AUG_DDIV((double)(float)S, 255.0);
    const double v = (double)(float)V;
    const int p = clip255((int)round(AUG_DMUL(v, AUG_DSUB(1.0, (double)fs))));
    const int q = clip255((int)round(AUG_DMUL(v, AUG_DSUB(1.0, (double)AUG_FMUL(fs, fr)))));
    const int t = clip255((int)round(AUG_DMUL(v, AUG_DSUB(1.0, (double)AUG_FMUL(fs, (float)AUG_DSUB(1.0, (double)fr))))));
    switch (i % 6) {
    case 0: r = V; g = t; b = p; break;
    case 1: r = q; g = V; b = p; break;
    case 2: r = p; g = V; b = t; break;
    case 3: r = p; g = q; b = V; break;
    case 4: r = t; g = p; b = V; break;
    default: r = V; g = p; b = q; break;
    }
}

AUG_FN void hue_shift(int &r, int &g, int &b, int shift) { hsv_round_trip(r, g, b, shift, false, 1.0f, 1.0f); }

// OP_HSV: hue shift, S factor `sat` and V factor `bright` in one round trip
AUG_FN void color_op(int op, int &r, int &g, int &b, float bright, float sat, int shift)
{
    if (op == OP_BRIGHTNESS) brightness(r, g, b, bright);
    else if (op == OP_SATURATION) saturation(r, g, b, sat);
    else hsv_round_trip(r, g, b, shift, op == OP_HSV, sat, bright);
}

// ---- addresses: window row / column -> source row / column, output column -> column of the resized row
AUG_FN int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// source row of window row y (column of window column x): under F_EDGE the window may leave the image and the border
// pixel is replicated; without it the window lies inside the image and the sum is the address
AUG_FN int src_row(int top, int y, int Hs, int flags) { return (flags & F_EDGE) ? clampi(top + y, 0, Hs - 1) : top + y; }
AUG_FN int src_col(int left, int x, int Ws, int flags) { return (flags & F_EDGE) ? clampi(left + x, 0, Ws - 1) : left + x; }

// column of the horizontally resized row (Wo wide) that output column xx shows: mirrored under F_FLIP
AUG_FN int stage1_col(int xx, int Wo, int flags) { return (flags & F_FLIP) ? Wo - 1 - xx : xx; }

}  // namespace yolo_aug
