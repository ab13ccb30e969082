"""Light sources and lighting filters as arguments of Engine.lighting (jh_lighting, the rule: DESIGN.md 5.14).

Every constructor returns a dict with a part of lighting's keywords: one of distant / point / spot names the light, one of diffuse /
specular the filter -- `engine.lighting(src, dst, **lighting.diffuse(surface_scale=5), **lighting.distant(45, 30))`,
`engine.capture(rec, lighting=dict(dst=image, **lighting.specular(exponent=20), **lighting.point(64, 64, 40)))`,
`engine.bevel(layer, target, a, b, 4, lighting.point(-50, -100, 200), (w, h))`.

jh_lighting takes a direction, the cosine of the cone angle and a LINEAR colour; the specification's azimuth, elevation,
limitingConeAngle and lighting-color (sRGB) are turned into those here, with Python's math: no trigonometry and no colour curve is in
the rule.  Coordinates are texels of the image, texel (X, Y) at (X + 0.5, Y + 0.5)."""
import math

from .imagecalls import LightKind, LightSource

WHITE = (1.0, 1.0, 1.0)


def srgb_to_linear(c):
    """The specification's decoding of one sRGB colour component in [0, 1]."""
    c = float(c)
    return c / 12.92 if c <= 0.04045 else ((c + 0.055) / 1.055) ** 2.4


def _color(color):
    r, g, b = color
    return (srgb_to_linear(r), srgb_to_linear(g), srgb_to_linear(b))


def distant(azimuth_deg, elevation_deg):
    """feDistantLight: the direction towards the light is (cos(azimuth) cos(elevation), sin(azimuth) cos(elevation), sin(elevation))."""
    az, el = math.radians(azimuth_deg), math.radians(elevation_deg)
    return dict(light=LightSource.DISTANT, direction=(math.cos(az) * math.cos(el), math.sin(az) * math.cos(el), math.sin(el)))


def point(x, y, z):
    """fePointLight at (x, y, z)."""
    return dict(light=LightSource.POINT, position=(float(x), float(y), float(z)))


def spot(x, y, z, points_at, exponent=1.0, limiting_cone_angle_deg=None):
    """feSpotLight at (x, y, z) pointing at `points_at` = (x, y, z); `exponent` is specularExponent of the light (the focus, in [1,
    128]); `limiting_cone_angle_deg`: no light beyond this angle from the axis (its sign is ignored; None: no cone)."""
    cone = -1.0 if limiting_cone_angle_deg is None else math.cos(math.radians(abs(limiting_cone_angle_deg)))
    px, py, pz = points_at
    return dict(light=LightSource.SPOT, position=(float(x), float(y), float(z)), points_at=(float(px), float(py), float(pz)),
                spot_exponent=float(exponent), cone_cos=cone)


def diffuse(surface_scale=1.0, kd=1.0, color=WHITE):
    """feDiffuseLighting: surfaceScale, diffuseConstant, lighting-color (sRGB components in [0, 1])."""
    return dict(kind=LightKind.DIFFUSE, surface_scale=float(surface_scale), constant=float(kd), color=_color(color))


def specular(surface_scale=1.0, ks=1.0, exponent=1.0, color=WHITE):
    """feSpecularLighting: surfaceScale, specularConstant, specularExponent in [1, 128], lighting-color (sRGB components in [0, 1])."""
    return dict(kind=LightKind.SPECULAR, surface_scale=float(surface_scale), constant=float(ks), specular_exponent=float(exponent), color=_color(color))
