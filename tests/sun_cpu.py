"""float64 numpy restatement of the directional sun's definitions (include/neusky_hip.h, "A directional sun"): the reference the
sun kernels and the frame render with `sun=` are tested against.  Nothing here imports the package."""
import numpy as np


def sun_direction(azimuth_deg, elevation_deg):
    az, el = np.radians(np.float64(azimuth_deg)), np.radians(np.float64(elevation_deg))
    return np.array([np.cos(az) * np.cos(el), np.sin(az) * np.cos(el), np.sin(el)])


def solid_angle(angular_diameter_deg):
    return 2.0 * np.pi * (1.0 - np.cos(np.radians(np.float64(angular_diameter_deg)) / 2.0))


def colour_from_radiance(radiance, angular_diameter_deg=0.533):
    return np.asarray(radiance, np.float64) * solid_angle(angular_diameter_deg) / (2.0 * np.pi)


def transfer(albedo, normals, weights, suns):
    """albedo, normals [R,S,3]; weights [R,S]; suns [K,3] -> t [K,R,3] and the tolerance scale sum_s |weights albedo| [R,3]"""
    a, n, w, s = (np.asarray(x, np.float64) for x in (albedo, normals, weights, suns))
    cos = np.clip(np.einsum("rsi,ki->krs", n, s), 0.0, 1.0)
    return np.einsum("krs,rs,rsc->krc", cos, w, a), np.einsum("rs,rsc->rc", np.abs(w), np.abs(a))


def shadow(vis, acc, acc_threshold, suns):
    """vis [K,R] or None, acc [R], suns [K,3] -> V [K,R]: 0 for a sun that has set and for a ray at or under the threshold"""
    s = np.asarray(suns, np.float64)
    K, R = s.shape[0], np.asarray(acc).shape[0]
    v = np.ones((K, R)) if vis is None else np.asarray(vis, np.float64)
    on = (s[:, 2] > 0.0)[:, None] & (np.asarray(acc, np.float64) > np.float64(acc_threshold))[None]
    return np.where(on, v, 0.0)


def linear_to_srgb(x):
    x = np.asarray(x, np.float64)
    return np.clip(np.where(x <= 0.0031308, 12.92 * x, 1.055 * np.abs(x) ** (1.0 / 2.4) - 0.055), 0.0, 1.0)


def composite(lin_sky, t, vis, acc, acc_threshold, suns, colours):
    """-> (rgb [K,R,3], lin [K,R,3], V [K,R])"""
    v = shadow(vis, acc, acc_threshold, suns)
    lin = np.asarray(lin_sky, np.float64)[None] + np.asarray(colours, np.float64)[:, None, :] * v[..., None] * np.asarray(t, np.float64)
    return linear_to_srgb(lin), lin, v
