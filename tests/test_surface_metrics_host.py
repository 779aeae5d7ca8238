"""Host checks of the HD95 / ASD path: the float64 restatement (tests/surface_reference.py) against values checked by hand and against scipy's
binary_erosion + distance_transform_edt (what MONAI runs); the C entry's declaration, export and argument checks, which fail before any launch."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (HERE, ROOT, os.path.join(ROOT, "nextgen-uia_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import surface_reference as R  # noqa: E402


def _pair(p, g):
    """bool masks [B,H,W] -> logits [B,2,H,W] whose arg-max is p, label [B,1,H,W] = g."""
    p, g = torch.as_tensor(p), torch.as_tensor(g)
    if p.dim() == 2:
        p, g = p[None], g[None]
    logits = torch.stack([torch.zeros(p.shape), p.float() * 2 - 1], 1)
    return logits, g.float()[:, None]


def _grid(*points, shape=(32, 32)):
    m = torch.zeros(shape, dtype=torch.bool)
    for y, x in points:
        m[y, x] = True
    return m


def _square(y0, x0, n, shape=(32, 32)):
    m = torch.zeros(shape, dtype=torch.bool)
    m[y0:y0 + n, x0:x0 + n] = True
    return m


# ------------------------------------------------------------------------------------------------ hand-checked values (32 x 32)
def test_two_single_pixels_are_a_3_4_5_triangle_apart():
    hd, asd = R.surface_distances(*_pair(_grid((3, 4)), _grid((6, 8))))
    assert hd[0] == 5.0 and asd[0] == 5.0


def test_a_square_against_itself_shifted_three_columns():
    hd, asd = R.surface_distances(*_pair(_square(5, 5, 10), _square(5, 8, 10)))
    assert hd[0] == 3.0 and asd[0] == 1.5


def test_full_images_have_their_outline_as_edge_and_distance_zero():
    full = torch.ones(32, 32, dtype=torch.bool)
    assert R.edges(full).sum() == 4 * 31 and not R.edges(full)[1:-1, 1:-1].any()
    hd, asd = R.surface_distances(*_pair(full, full))
    assert hd[0] == 0.0 and asd[0] == 0.0


def test_empty_masks_are_not_finite():
    sq, empty = _square(4, 4, 6), torch.zeros(32, 32, dtype=torch.bool)
    for p, g in ((empty, sq), (sq, empty), (empty, empty)):
        hd, asd = R.surface_distances(*_pair(p, g))
        assert not np.isfinite(hd[0]) and not np.isfinite(asd[0])
    hd, asd = R.surface_distances(*_pair(empty, empty))
    assert math.isnan(hd[0]) and math.isnan(asd[0])


def test_masks_follow_torch_argmax_ties_and_nans():
    logits = torch.tensor([[1.0, 1.0], [0.0, float("nan")], [float("nan"), 5.0], [float("nan"), float("nan")], [2.0, 3.0]]).T.reshape(1, 2, 1, 5)
    P, _ = R.masks(logits, torch.zeros(1, 1, 1, 5))
    assert P[0, 0].tolist() == [False, True, False, False, True]


def test_percentile_zero_is_the_maximum_as_in_monai():
    d = torch.tensor([1.0, 2.0, 7.0], dtype=torch.float32)
    assert R.quantile(d, 0) == 7.0 and R.quantile(d, 100) == 7.0 and R.quantile(d, 50) == 2.0


# ------------------------------------------------------------------------------------------------ against scipy (MONAI's host path)
def _scipy(P, G, percentile):
    from scipy.ndimage import binary_erosion, distance_transform_edt
    hd, asd = [], []
    for p, g in zip(P.numpy(), G.numpy()):
        if not p.any() or not g.any():
            hd.append(np.nan)
            asd.append(np.nan)
            continue
        ep, eg = p ^ binary_erosion(p), g ^ binary_erosion(g)
        d_pg = torch.from_numpy(distance_transform_edt(~eg)[ep].astype(np.float32))
        d_gp = torch.from_numpy(distance_transform_edt(~ep)[eg].astype(np.float32))
        q = (lambda d: float(d.max())) if not percentile else (lambda d: float(torch.quantile(d, percentile / 100)))
        hd.append(max(q(d_pg), q(d_gp)))
        asd.append(float(d_pg.double().mean()))
    return np.array(hd), np.array(asd)


def _blobs(B, H, W, seed, k=3):
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    out = torch.zeros(B, H, W, dtype=torch.bool)
    for b in range(B):
        for _ in range(k):
            cy, cx = float(torch.rand(1, generator=g)) * H, float(torch.rand(1, generator=g)) * W
            ry, rx = 1 + float(torch.rand(1, generator=g)) * H / 3, 1 + float(torch.rand(1, generator=g)) * W / 3
            out[b] |= ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1
    return out


@pytest.mark.parametrize("case", ["blobs", "noise", "border", "non_square", "thin"])
@pytest.mark.parametrize("percentile", [0, 50, 95, 100])
def test_restatement_matches_scipy(case, percentile):
    pytest.importorskip("scipy")
    g = torch.Generator().manual_seed(11)
    if case == "blobs":
        P, G = _blobs(4, 48, 48, 1), _blobs(4, 48, 48, 2)
    elif case == "noise":
        P, G = torch.rand(3, 40, 40, generator=g) > 0.5, _blobs(3, 40, 40, 3)
        G[1] = torch.rand(40, 40, generator=g) > 0.7
    elif case == "border":
        P, G = _blobs(3, 36, 36, 4, k=6), torch.ones(3, 36, 36, dtype=torch.bool)
        G[1, 10:20, 10:20] = False
        P[2] = True
    elif case == "non_square":
        P, G = _blobs(4, 24, 70, 5), _blobs(4, 24, 70, 6)
    else:
        P, G = torch.zeros(3, 1, 50, dtype=torch.bool), torch.zeros(3, 1, 50, dtype=torch.bool)
        P[:, 0, 3:9] = True
        G[:, 0, 30:] = True
        G[2, 0, 5] = True
    want_hd, want_asd = _scipy(P, G, percentile)
    hd, asd = R.surface_distances(*_pair(P, G), percentile=percentile)
    assert np.array_equal(np.isfinite(hd), np.isfinite(want_hd)) and np.array_equal(np.isfinite(asd), np.isfinite(want_asd))
    f = np.isfinite(want_hd)
    assert np.array_equal(hd[f], want_hd[f])
    assert np.allclose(asd[f], want_asd[f], rtol=1e-12, atol=0)


# ------------------------------------------------------------------------------------------------ the C entry without a GPU
def test_surface_entry_is_declared_exported_and_typed():
    from uia_hip import _lib
    src = open(os.path.join(ROOT, "include", "uia_hip.h")).read()
    assert "uia_surface_distances_workspace_bytes(int B, int H, int W)" in src and "int uia_surface_distances(void* stream" in src
    handle = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(handle, "uia_surface_distances") and hasattr(handle, "uia_surface_distances_workspace_bytes")
    assert "uia_surface_distances" in _lib.PROTOTYPES and "uia_surface_distances_workspace_bytes" in _lib.PROTOTYPES


def test_surface_argument_checks_fail_before_any_launch():
    from uia_hip import _lib
    lib = _lib.lib()
    need = lib.uia_surface_distances_workspace_bytes(2, 16, 16)
    assert need >= 2 * 16 * 16 * 14 and lib.uia_surface_distances_workspace_bytes(0, 16, 16) == 0
    fake = 4096                                                  # never dereferenced: every case below is refused by the argument checks

    def call(B=2, H=16, W=16, logits=fake, label=fake, pct=95.0, ws=fake, ws_bytes=need, hd=fake, asd=fake):
        return lib.uia_surface_distances(None, B, H, W, logits, label, pct, ws, ws_bytes, hd, asd)

    for kw, text in ((dict(logits=None), b"null"), (dict(label=None), b"null"), (dict(ws=None), b"null"), (dict(hd=None), b"null"),
                     (dict(asd=None), b"null"), (dict(H=0), b"bad shape"), (dict(W=1025), b"bad shape"), (dict(B=0), b"bad shape"),
                     (dict(pct=101.0), b"percentile"), (dict(pct=-1.0), b"percentile"), (dict(pct=float("nan")), b"percentile"),
                     (dict(ws_bytes=need - 1), b"workspace")):
        assert call(**kw) != 0, kw
        msg = lib.uia_last_error()
        assert b"uia_surface_distances" in msg and text in msg, (kw, msg)


def test_surface_op_refuses_cpu_tensors():
    from uia_hip import ops
    from uia_hip._lib import UiaError
    logits, label = _pair(_square(2, 2, 4), _square(3, 3, 4))
    with pytest.raises(UiaError):
        ops.surface_distances(logits, label)
