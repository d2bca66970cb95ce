"""NumPy restatement of the communication channels' verdict (csrc/channel_rows.hpp: channel_verdict): whether a message sender -> recipient
arrives.  tests/test_channel_host.py ties it to the reference's recorded sent -> delivered matrices (tests/golden/channel_*.npz); the GPU tests
take their expected verdicts from it."""
import numpy as np


def binomial_one(rate, u):
    """The project's rule for binomial(1, p) of a uniform u (make_golden.py RecordingRNG.binomial): 1 iff u > 1 - p where p <= 0.5, else iff u <= p."""
    u = np.asarray(u, dtype=np.float64)
    return (u > 1.0 - rate) if rate <= 0.5 else (u <= rate)


def pair_distances(positions):
    """[..., n, 2] locations -> [..., n, n] distances [sender][recipient]: np.linalg.norm of the difference (entities.py:91-94)."""
    p = np.asarray(positions, dtype=np.float64)
    d = p[..., None, :, :] - p[..., :, None, :]
    return np.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1])


def channel_verdict(disabled, limit, rate, mask, u, positions):
    """[..., n, n] bool [sender][recipient]: the message arrives.  `limit` None / negative / inf: none; `mask` None or [..., n, n], non-zero = deliver;
    `u` [..., n, n] uniforms (NaN where none was drawn: no draw drops nothing); `positions` [..., n, 2]."""
    u = np.asarray(u, dtype=np.float64)
    keep = np.ones(u.shape, dtype=bool)
    if disabled:
        keep[...] = False
    if limit is not None and limit >= 0.0 and np.isfinite(limit):
        keep &= pair_distances(positions) <= limit
    if rate > 0.0:
        with np.errstate(invalid='ignore'):
            keep &= ~binomial_one(rate, u)
    if mask is not None:
        keep &= np.asarray(mask) != 0
    return keep
