"""What the forward/backward tests share (test infrastructure): random monotone tunnels, the cells inside a band, and the
environment switches that force a schedule."""
import numpy as np

from pagan2_msa_amd import abi

ENV_VARS = ("PAGAN_FB_DEEP", "PAGAN_FB_DEEP_MIN_ND", "PAGAN_FB_RING", "PAGAN_FB_RING_MIN_ND", "PAGAN_FB_BAND_MIN_ND", "PAGAN_FB_GROUPS")


def set_env(monkeypatch, env):
    """every schedule switch cleared, then `env` ({name: value}) set"""
    for v in ENV_VARS:
        monkeypatch.delenv(v, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def random_tunnel(rng, Lx, Ly, lo_half, hi_half):
    """a monotone band around the main diagonal whose half-width is drawn per row from [lo_half, hi_half)"""
    half = rng.integers(lo_half, hi_half, Lx)
    centre = np.arange(Lx) * (Ly - 1) // max(Lx - 1, 1)
    upper = np.maximum.accumulate(np.maximum(centre - half, 0))
    lower = np.maximum.accumulate(np.minimum(centre + half, Ly - 1))
    upper[0] = 0
    lower[-1] = Ly - 1
    return abi.Band(upper.astype(np.int32), lower.astype(np.int32))


def in_band(Lx, Ly, band):
    """[Lx, Ly] bool: the cells inside the tunnel as the library clamps it (no band: all)"""
    if band is None:
        return np.ones((Lx, Ly), bool)
    lo, hi = np.maximum(band.upper, 0), np.minimum(band.lower, Ly - 1)
    j = np.arange(Ly)[None, :]
    return (j >= lo[:, None]) & (j <= hi[:, None])
