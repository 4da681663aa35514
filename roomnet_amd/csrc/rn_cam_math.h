// The per-pixel arithmetic of the grad-CAM heat map (rn_cam_overlay.hip): roomnet_amd/cam.py's upsample,
// colormap and overlay for ONE pixel, in float64, in that file's order of operations and without contraction (every product and
// sum is rounded on its own, as NumPy rounds them), so that the bytes are cam.overlay_image's.  Device functions only; the file
// includes nothing, so that tools/cam_overlay_main.cpp can compile the same text for the host and compare it with cam.py.
//
// Plain operators under `fp contract(off)`, NOT __dmul_rn / __dadd_rn: the compiler's header defines those as `x * y` and `x + y`
// compiled with contraction allowed, and inlined into a sum of products they were fused (seen on an MI355X: one byte of the
// 16 x 16 test image at weight 0.3, where (1 - w) * image + w * heat is no longer exact).  The pragma holds to the end of the
// translation unit that includes this file.  Division is IEEE (its expansion's own fused steps are part of a correctly rounded
// quotient), rint rounds half to even.
#pragma once
#pragma clang fp contract(off)

// the blue -> cyan -> green -> yellow -> red ramp of cam.py (_ANCHORS_BGR), anchors at 0, 1/4, ... 1
static __constant__ double rn_cam_anchors[5][3] = {{128, 0, 0}, {255, 255, 0}, {0, 255, 0}, {0, 255, 255}, {0, 0, 255}};

// cam.upsample's axis(): output sample i of an axis of n_in map samples, scale = n_in / double(side)
struct rn_cam_axis {
    int lo, hi;
    double frac;
};
__device__ __forceinline__ rn_cam_axis rn_cam_axis_of(int i, int n_in, double scale) {
    double src = (static_cast<double>(i) + 0.5) * scale - 0.5;
    src = fmin(fmax(src, 0.0), static_cast<double>(n_in - 1));
    const double fl = floor(src);
    rn_cam_axis a;
    a.lo = static_cast<int>(fl);
    a.hi = a.lo + 1 < n_in ? a.lo + 1 : n_in - 1;
    a.frac = src - fl;
    return a;
}

// the upsampled, clamped value at (y, x); never -0.0, so that its bits order like the value
__device__ __forceinline__ double rn_cam_up(const float* __restrict__ map, int mw, const rn_cam_axis& y, const rn_cam_axis& x) {
    const float* r0 = map + static_cast<long long>(y.lo) * mw;
    const float* r1 = map + static_cast<long long>(y.hi) * mw;
    const double omx = 1.0 - x.frac, omy = 1.0 - y.frac;
    const double top = static_cast<double>(r0[x.lo]) * omx + static_cast<double>(r0[x.hi]) * x.frac;
    const double bot = static_cast<double>(r1[x.lo]) * omx + static_cast<double>(r1[x.hi]) * x.frac;
    const double up = top * omy + bot * y.frac;
    return up > 0.0 ? up : 0.0;
}

// cam.upsample's normalisation to float32, then cam.colormap: the heat colour (BGR, integral values 0..255) of an upsampled value
// under the map's maximum mx (mx <= 0: the all-zero map, the ramp's first anchor)
__device__ __forceinline__ void rn_cam_heat(double up, double mx, double (&heat)[3]) {
    const float v = mx > 0.0 ? static_cast<float>(up / mx) : 0.0f;
    const double v64 = fmin(fmax(static_cast<double>(v), 0.0), 1.0) * 4.0;
    const double fl = fmin(floor(v64), 3.0);
    const int i = static_cast<int>(fl);
    const double t = v64 - fl, omt = 1.0 - t;
#pragma unroll
    for (int k = 0; k < 3; ++k) heat[k] = rint(rn_cam_anchors[i][k] * omt + rn_cam_anchors[i + 1][k] * t);
}

// cam.overlay's blend of one channel: clip(rint((1 - weight) * im + weight * heat), 0, 255); `omw` is 1.0 - weight
__device__ __forceinline__ unsigned rn_cam_blend(unsigned im, double heat, double weight, double omw) {
    const double r = rint(omw * static_cast<double>(im) + weight * heat);
    return static_cast<unsigned>(fmin(fmax(r, 0.0), 255.0));
}
