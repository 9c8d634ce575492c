"""Host side of the shaded previews (capi.Model.render / render_posed, StageIISolver.render, mosh_head.stageii_preview): a camera that
frames a sequence, and contact sheets.  NumPy only; no device, no imaging library."""
from __future__ import annotations

import numpy as np

VIEWS = {'front': (0.0, 0.0), 'back': (180.0, 0.0), 'left': (90.0, 0.0), 'right': (-90.0, 0.0), 'top': (0.0, 90.0)}
OBSERVED_RGB = (215, 48, 39)      # observed markers
SIMULATED_RGB = (44, 101, 201)    # the solve's simulated markers


def _toward_camera(azimuth_deg, elevation_deg, up):
    """Unit vector from the subject to the camera.  up = 'z': azimuth 0 stands at -y and looks along +y; up = 'y': azimuth 0 stands at
    +z and looks along -z (the bodies' rest pose faces +z); positive azimuth walks towards +x, positive elevation rises."""
    az, el = np.deg2rad(float(azimuth_deg)), np.deg2rad(float(elevation_deg))
    if up == 'z':
        return np.array([np.cos(el) * np.sin(az), -np.cos(el) * np.cos(az), np.sin(el)])
    return np.array([np.cos(el) * np.sin(az), np.sin(el), np.cos(el) * np.cos(az)])


def preview_camera(joints, size, view='front', up='z', margin=1.15):
    """One fixed capi.Camera for a whole sequence: it looks at the centre of the bounding box of joints[F, K, 3] (or [K, 3]) from the
    direction `view` -- 'front' | 'back' | 'left' | 'right' | 'top' or (azimuth_deg, elevation_deg) -- with the world axis `up`
    ('z' | 'y') pointing up in the image, from the smallest distance at which the box, grown by `margin` about its centre, lies inside
    the image of size = (width, height); focal length max(width, height) pixels, principal point at the image centre; znear is a tenth
    of the distance to the nearest corner of that box."""
    from . import capi
    j = np.asarray(joints, dtype=np.float64).reshape(-1, 3)
    if j.size == 0 or not np.isfinite(j).all():
        raise ValueError('preview_camera: joints must be finite and not empty')
    try:
        W, H = (int(x) for x in size)
    except (TypeError, ValueError):
        raise ValueError(f'preview_camera: size must be (width, height), got {size!r}')
    if W < 1 or H < 1:
        raise ValueError(f'preview_camera: size must be positive, got {size!r}')
    if up not in ('z', 'y'):
        raise ValueError(f"preview_camera: up must be 'z' or 'y', got {up!r}")
    if not float(margin) >= 1.0:
        raise ValueError(f'preview_camera: margin must be >= 1, got {margin!r}')
    if isinstance(view, str):
        if view not in VIEWS:
            raise ValueError(f'preview_camera: view must be one of {sorted(VIEWS)} or (azimuth_deg, elevation_deg), got {view!r}')
        az, el = VIEWS[view]
    else:
        try:
            az, el = (float(x) for x in view)
        except (TypeError, ValueError):
            raise ValueError(f'preview_camera: view must be one of {sorted(VIEWS)} or (azimuth_deg, elevation_deg), got {view!r}')
    d = _toward_camera(az, el, up)
    fwd = -d
    world_up = np.array([0.0, 0.0, 1.0]) if up == 'z' else np.array([0.0, 1.0, 0.0])
    ref = world_up
    if abs(fwd @ world_up) > 0.999:            # looking straight down or up: the image's up is where the azimuth's level view looks
        ref = -_toward_camera(az, 0.0, up) * np.sign(-(fwd @ world_up))
    right = np.cross(fwd, ref)
    right /= np.linalg.norm(right)
    down = np.cross(fwd, right)
    R = np.stack([right, down, fwd])
    lo, hi = j.min(0), j.max(0)
    centre = 0.5 * (lo + hi)
    half = np.maximum(0.5 * (hi - lo) * float(margin), 1e-3)
    corners = centre + half * np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], dtype=np.float64)
    rel = (corners - centre) @ R.T             # the corners in camera axes, about the centre
    focal = float(max(W, H))
    dist = max(np.max(2.0 * focal * np.abs(rel[:, 0]) / W - rel[:, 2]), np.max(2.0 * focal * np.abs(rel[:, 1]) / H - rel[:, 2]))
    dist = max(dist, np.max(-rel[:, 2]) + 1e-2)
    eye = centre + dist * d
    nearest = np.min(rel[:, 2]) + dist
    return capi.Camera.make(R, -R @ eye, focal, focal, 0.5 * W, 0.5 * H, 0.1 * nearest)


def project(camera, points):
    """(u, v, z) of world points[..., 3] through a capi.Camera, in NumPy f64 (pixels, pixels, metres)."""
    c = camera.as_dict() if hasattr(camera, 'as_dict') else camera
    x = np.asarray(points, dtype=np.float64) @ np.asarray(c['R']).T + np.asarray(c['t'])
    return c['fx'] * x[..., 0] / x[..., 2] + c['cx'], c['fy'] * x[..., 1] / x[..., 2] + c['cy'], x[..., 2]


def contact_sheet(images, columns, fill=255):
    """images[n, H, W, 3] (uint8) side by side, `columns` a row, row by row; the cells behind the last image hold `fill`."""
    imgs = np.asarray(images)
    if imgs.ndim != 4 or imgs.shape[3] != 3 or imgs.dtype != np.uint8 or imgs.shape[0] < 1:
        raise ValueError(f'contact_sheet: images must be uint8 [n >= 1, H, W, 3], got {imgs.dtype} {tuple(imgs.shape)}')
    columns = int(columns)
    if columns < 1:
        raise ValueError(f'contact_sheet: columns must be >= 1, got {columns}')
    n, H, W = imgs.shape[:3]
    columns = min(columns, n)
    rows = (n + columns - 1) // columns
    sheet = np.full((rows * H, columns * W, 3), fill, dtype=np.uint8)
    for i in range(n):
        r, c = divmod(i, columns)
        sheet[r * H:(r + 1) * H, c * W:(c + 1) * W] = imgs[i]
    return sheet
