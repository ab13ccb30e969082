// blend_rule.h -- shared/blend.wgsl as the one text of the blend arithmetic: the sixteen mix modes, the fourteen Porter-Duff operators
// and blend_rule(), the body of blend_mix_compose (blend.wgsl:288-310).  Included by kernels_fine.hip (END_CLIP: its noinline
// wrapper makes `mode` a scalar and calls blend_rule) and by kernels_composite.hip (jh_composite, DESIGN.md 5.8: image onto image),
// so the two cannot drift apart.  Only + - * /, sqrtf and the min / max / abs / mix of dmath.h: every operation binary32, rounded
// once, no contraction (the build's -ffp-contract=off).  tests/composite_ref.py restates it in numpy; tests/test_blend_spec.py and
// tests/test_composite_spec.py hold it to the W3C formulas.
// Everything sits in the unnamed namespace, like the rest of a kernel file's device functions: internal to the file that includes it.
#pragma once
#include "dmath.h"

namespace {

struct V4 {
    float x, y, z, w;
};
struct V3 {
    float x, y, z;
};
JD V4 v4(float x, float y, float z, float w) { V4 r; r.x = x; r.y = y; r.z = z; r.w = w; return r; }
JD V3 v3(float x, float y, float z) { V3 r; r.x = x; r.y = y; r.z = z; return r; }

// ---- shared/blend.wgsl ----
JD V3 screen(V3 cb, V3 cs) { return v3(cb.x + cs.x - (cb.x * cs.x), cb.y + cs.y - (cb.y * cs.y), cb.z + cs.z - (cb.z * cs.z)); }
JD float color_dodge(float cb, float cs) {
    if (cb == 0.0f) return 0.0f; else if (cs == 1.0f) return 1.0f; else return jd::fmin_(1.0f, cb / (1.0f - cs));
}
JD float color_burn(float cb, float cs) {
    if (cb == 1.0f) return 1.0f; else if (cs == 0.0f) return 0.0f; else return 1.0f - jd::fmin_(1.0f, (1.0f - cb) / cs);
}
JD float hard_light1(float cb, float cs) {
    float scr_cs = 2.0f * cs - 1.0f;
    float a = cb + scr_cs - (cb * scr_cs);
    float b = cb * 2.0f * cs;
    return (cs <= 0.5f) ? b : a;
}
JD V3 hard_light(V3 cb, V3 cs) { return v3(hard_light1(cb.x, cs.x), hard_light1(cb.y, cs.y), hard_light1(cb.z, cs.z)); }
JD float soft_light1(float cb, float cs) {
    float d = (cb <= 0.25f) ? (((16.0f * cb - 12.0f) * cb + 4.0f) * cb) : jd::sqrt_(cb);
    float t = cb + (2.0f * cs - 1.0f) * (d - cb);
    float f = cb - (1.0f - 2.0f * cs) * cb * (1.0f - cb);
    return (cs <= 0.5f) ? f : t;
}
JD V3 soft_light(V3 cb, V3 cs) { return v3(soft_light1(cb.x, cs.x), soft_light1(cb.y, cs.y), soft_light1(cb.z, cs.z)); }
JD float sat(V3 c) { return jd::fmax_(c.x, jd::fmax_(c.y, c.z)) - jd::fmin_(c.x, jd::fmin_(c.y, c.z)); }
JD float lum(V3 c) { return c.x * 0.3f + c.y * 0.59f + c.z * 0.11f; }
JD V3 clip_color(V3 c) {
    float l = lum(c);
    float n = jd::fmin_(c.x, jd::fmin_(c.y, c.z));
    float x = jd::fmax_(c.x, jd::fmax_(c.y, c.z));
    if (n < 0.0f) c = v3(l + (((c.x - l) * l) / (l - n)), l + (((c.y - l) * l) / (l - n)), l + (((c.z - l) * l) / (l - n)));
    if (x > 1.0f) c = v3(l + (((c.x - l) * (1.0f - l)) / (x - l)), l + (((c.y - l) * (1.0f - l)) / (x - l)), l + (((c.z - l) * (1.0f - l)) / (x - l)));
    return c;
}
JD V3 set_lum(V3 c, float l) { float d = l - lum(c); return clip_color(v3(c.x + d, c.y + d, c.z + d)); }
JD void set_sat_inner(float& cmin, float& cmid, float& cmax, float s) {
    if (cmax > cmin) { cmid = ((cmid - cmin) * s) / (cmax - cmin); cmax = s; }
    else { cmid = 0.0f; cmax = 0.0f; }
    cmin = 0.0f;
}
JD V3 set_sat(V3 c, float s) {
    float r = c.x, g = c.y, b = c.z;
    if (r <= g) {
        if (g <= b) set_sat_inner(r, g, b, s);
        else { if (r <= b) set_sat_inner(r, b, g, s); else set_sat_inner(b, r, g, s); }
    } else {
        if (r <= b) set_sat_inner(g, r, b, s);
        else { if (g <= b) set_sat_inner(g, b, r, s); else set_sat_inner(b, g, r, s); }
    }
    return v3(r, g, b);
}
JD V3 blend_mix(V3 cb, V3 cs, uint32_t mode) {  // blend.wgsl:142-195
    switch (mode) {
        case 1: return v3(cb.x * cs.x, cb.y * cs.y, cb.z * cs.z);
        case 2: return screen(cb, cs);
        case 3: return hard_light(cs, cb);
        case 4: return v3(jd::fmin_(cb.x, cs.x), jd::fmin_(cb.y, cs.y), jd::fmin_(cb.z, cs.z));
        case 5: return v3(jd::fmax_(cb.x, cs.x), jd::fmax_(cb.y, cs.y), jd::fmax_(cb.z, cs.z));
        case 6: return v3(color_dodge(cb.x, cs.x), color_dodge(cb.y, cs.y), color_dodge(cb.z, cs.z));
        case 7: return v3(color_burn(cb.x, cs.x), color_burn(cb.y, cs.y), color_burn(cb.z, cs.z));
        case 8: return hard_light(cb, cs);
        case 9: return soft_light(cb, cs);
        case 10: return v3(jd::abs_(cb.x - cs.x), jd::abs_(cb.y - cs.y), jd::abs_(cb.z - cs.z));
        case 11: return v3(cb.x + cs.x - 2.0f * cb.x * cs.x, cb.y + cs.y - 2.0f * cb.y * cs.y, cb.z + cs.z - 2.0f * cb.z * cs.z);
        case 12: return set_lum(set_sat(cs, sat(cb)), lum(cb));
        case 13: return set_lum(set_sat(cb, sat(cs)), lum(cb));
        case 14: return set_lum(cs, lum(cb));
        case 15: return set_lum(cb, lum(cs));
        default: return cs;
    }
}
JD V4 blend_compose(V3 cb, V3 cs, float ab, float as_, uint32_t mode) {  // blend.wgsl:216-284
    float fa = 0.0f, fb = 0.0f;
    switch (mode) {
        case 1: fa = 1.0f; fb = 0.0f; break;
        case 2: fa = 0.0f; fb = 1.0f; break;
        case 0: fa = 1.0f; fb = 1.0f - as_; break;
        case 4: fa = 1.0f - ab; fb = 1.0f; break;
        case 5: fa = ab; fb = 0.0f; break;
        case 6: fa = 0.0f; fb = as_; break;
        case 7: fa = 1.0f - ab; fb = 0.0f; break;
        case 8: fa = 0.0f; fb = 1.0f - as_; break;
        case 9: fa = ab; fb = 1.0f - as_; break;
        case 10: fa = 1.0f - ab; fb = as_; break;
        case 11: fa = 1.0f - ab; fb = 1.0f - as_; break;
        case 12: fa = 1.0f; fb = 1.0f; break;
        case 13:
            return v4(jd::fmin_(1.0f, as_ * cs.x + ab * cb.x), jd::fmin_(1.0f, as_ * cs.y + ab * cb.y), jd::fmin_(1.0f, as_ * cs.z + ab * cb.z),
                      jd::fmin_(1.0f, as_ + ab));
        default: break;
    }
    float as_fa = as_ * fa;
    float ab_fb = ab * fb;
    return v4(as_fa * cs.x + ab_fb * cb.x, as_fa * cs.y + ab_fb * cb.y, as_fa * cs.z + ab_fb * cb.z, jd::fmin_(as_fa + ab_fb, 1.0f));
}
// blend_mix_compose of blend.wgsl:288-310 on premultiplied (colour, alpha) pairs; mode = mix << 8 | compose (bit 15, the WGSL's
// "clip" flag of Mix.Clip, is masked for the fast arm as the WGSL does).  The first arm is Normal + SrcOver.
JD V4 blend_rule(V4 backdrop, V4 src, uint32_t mode) {
    const float EPSILON = 1e-15f;
    if ((mode & 0x7fffu) == 0u) {
        float k = 1.0f - src.w;
        return v4(backdrop.x * k + src.x, backdrop.y * k + src.y, backdrop.z * k + src.z, backdrop.w * k + src.w);
    }
    float inv_src_a = 1.0f / jd::fmax_(src.w, EPSILON);
    V3 cs = v3(src.x * inv_src_a, src.y * inv_src_a, src.z * inv_src_a);
    float inv_backdrop_a = 1.0f / jd::fmax_(backdrop.w, EPSILON);
    V3 cb = v3(backdrop.x * inv_backdrop_a, backdrop.y * inv_backdrop_a, backdrop.z * inv_backdrop_a);
    uint32_t mix_mode = mode >> 8;
    V3 mixed = blend_mix(cb, cs, mix_mode);
    cs = v3(jd::mix_(cs.x, mixed.x, backdrop.w), jd::mix_(cs.y, mixed.y, backdrop.w), jd::mix_(cs.z, mixed.z, backdrop.w));
    uint32_t compose_mode = mode & 0xffu;
    if (compose_mode == 0u) {
        return v4(jd::mix_(backdrop.x, cs.x, src.w), jd::mix_(backdrop.y, cs.y, src.w), jd::mix_(backdrop.z, cs.z, src.w), src.w + backdrop.w * (1.0f - src.w));
    }
    return blend_compose(cb, cs, backdrop.w, src.w, compose_mode);
}

}  // namespace
