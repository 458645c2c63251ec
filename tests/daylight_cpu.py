"""float64 numpy restatement of the clear-sky daylight model's definitions (include/neusky_hip.h, "A clear-sky daylight model"; Preetham,
Shirley, Smits 1999): the reference the daylight kernel, relight.DaylightSky and the frame render with `daylight=` are tested against.
Written from the definitions; nothing here imports the package."""
import numpy as np

PEREZ = {  # (A, B, C, D, E) as (slope, offset) in T
    "Y": ((0.1787, -1.4630), (-0.3554, 0.4275), (-0.0227, 5.3251), (0.1206, -2.5771), (-0.0670, 0.3703)),
    "x": ((-0.0193, -0.2592), (-0.0665, 0.0008), (-0.0004, 0.2125), (-0.0641, -0.8989), (-0.0033, 0.0452)),
    "y": ((-0.0167, -0.2608), (-0.0950, 0.0092), (-0.0079, 0.2102), (-0.0441, -1.6537), (-0.0109, 0.0529)),
}
MX = np.array([[0.00166, -0.00375, 0.00209, 0.0], [-0.02903, 0.06377, -0.03202, 0.00394], [0.11693, -0.21196, 0.06052, 0.25886]])
MY = np.array([[0.00275, -0.00610, 0.00317, 0.0], [-0.04214, 0.08970, -0.04153, 0.00516], [0.15346, -0.26756, 0.06670, 0.26688]])
XYZ_TO_RGB = np.array([[3.2404542, -1.5371385, -0.4985314], [-0.9692660, 1.8760108, 0.0415560], [0.0556434, -0.2040259, 1.0572252]])
WAVELENGTHS_UM = np.array([0.610, 0.550, 0.465])
SOLAR_ILLUMINANCE_KLX = 133.1


def sun_direction(azimuth_deg, elevation_deg):
    az, el = np.radians(np.float64(azimuth_deg)), np.radians(np.float64(elevation_deg))
    return np.array([np.cos(az) * np.cos(el), np.sin(az) * np.cos(el), np.sin(el)])


def coefficients(T, which):
    return [np.float64(a) * np.float64(T) + np.float64(b) for a, b in PEREZ[which]]


def perez(T, which, ct, g):
    """F(ct, g) of one of "Y", "x", "y"; ct >= 0"""
    A, B, C, D, E = coefficients(T, which)
    ct = np.asarray(ct, np.float64)
    with np.errstate(divide="ignore", over="ignore"):
        a = np.where(ct > 0.0, np.exp(B / np.where(ct > 0.0, ct, 1.0)), 0.0)
    return (1.0 + A * a) * (1.0 + C * np.exp(D * g) + E * np.cos(g) ** 2)


def zenith(T, ts):
    """(Yz, xz, yz) of a sun at zenith angle ts"""
    T, ts = np.float64(T), np.float64(ts)
    chi = (4.0 / 9.0 - T / 120.0) * (np.pi - 2.0 * ts)
    Yz = (4.0453 * T - 4.9710) * np.tan(chi) - 0.2155 * T + 2.4192
    tv, sv = np.array([T * T, T, 1.0]), np.array([ts ** 3, ts ** 2, ts, 1.0])
    return Yz, tv @ MX @ sv, tv @ MY @ sv


def sky_Yxy(T, sun, directions):
    """sun [3] (s.z > 0), directions [N,3] -> (Y, x, y, below) [N]: the sky towards each direction's point on or above the horizon"""
    s = np.asarray(sun, np.float64)
    d = np.array(directions, np.float64).reshape(-1, 3)
    below = d[:, 2] < 0.0
    down = below & (d[:, 0] == 0.0) & (d[:, 1] == 0.0)
    d[below, 2] = 0.0
    d[down, 2] = 1.0
    d = d / np.linalg.norm(d, axis=1, keepdims=True)
    ct = d[:, 2]
    g = np.arctan2(np.linalg.norm(np.cross(d, s[None]), axis=1), d @ s)
    ts = np.arccos(np.clip(s[2], -1.0, 1.0))
    out = []
    for which, zen in zip(("Y", "x", "y"), zenith(T, ts)):
        out.append(zen * perez(T, which, ct, g) / perez(T, which, 1.0, ts))
    return out[0], out[1], out[2], below


def radiance(T, suns, directions, exposure=1.0, ground=(1.0, 1.0, 1.0), clamp=True):
    """suns [K,3], directions [N,3] -> linear sRGB [K,N,3]"""
    suns = np.asarray(suns, np.float64).reshape(-1, 3)
    d = np.asarray(directions, np.float64).reshape(-1, 3)
    out = np.zeros((suns.shape[0], d.shape[0], 3))
    for k, s in enumerate(suns):
        if not s[2] > 0.0:
            continue  # a sun that has set: its whole sky is 0
        n2 = (d * d).sum(axis=1)
        none = ~((n2 > 0.0) & np.isfinite(n2))  # no direction: no sky
        Y, x, y, below = sky_Yxy(T, s, np.where(none[:, None], np.array([0.0, 0.0, 1.0]), d))
        XYZ = np.stack([x * Y / y, Y, (1.0 - x - y) * Y / y], axis=-1)
        rgb = XYZ @ XYZ_TO_RGB.T
        if clamp:
            rgb = np.maximum(rgb, 0.0)
        rgb = rgb * np.float64(exposure)
        out[k] = np.where(none[:, None], 0.0, np.where(below[:, None], rgb * np.asarray(ground, np.float64)[None], rgb))
    return out


def transmittance(T, elevation_deg):
    """tau [3] of the direct sun at the three wavelengths: Rayleigh and aerosol (Angstrom) extinction along the relative air mass"""
    ts = np.radians(90.0 - np.float64(elevation_deg))
    m = 1.0 / (np.cos(ts) + 0.15 * (93.885 - np.degrees(ts)) ** -1.253)
    beta = 0.04608 * np.float64(T) - 0.04586
    return np.exp(-0.008735 * WAVELENGTHS_UM ** -4.08 * m) * np.exp(-beta * WAVELENGTHS_UM ** -1.3 * m)


def sun_colour(T, elevation_deg, exposure=1.0):
    """C [3] = exposure (133.1 / 2 pi) tau; 0 for a sun that has set"""
    if not np.sin(np.radians(np.float64(elevation_deg))) > 0.0:
        return np.zeros(3)
    return np.float64(exposure) * SOLAR_ILLUMINANCE_KLX / (2.0 * np.pi) * transmittance(T, elevation_deg)
