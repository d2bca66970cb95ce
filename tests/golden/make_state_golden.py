#!/usr/bin/env python3
"""Generator of tests/golden/state_norm.npz: the reference's own normalised global state for one recorded trace per entity shape.

Imports the upstream reference read-only (its checkout is named by the MATE_REFERENCE environment variable) under the `gymshim`
package next to this file, and stores, for every trace below: the trace's name, `env.state_space.low / high` of the reference
environment the trace's scenario builds, and `mate.normalize_observation(state, env.state_space)` (mate/agents/utils.py:97-127) of the
trace's recorded `reset/state` and `step/state` rows -- f64, at most the first 64 steps of a trace.  Arrays and names only: data, no
program text.

    MATE_REFERENCE=<checkout of XuehaiPan/mate> python tests/golden/make_state_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'gymshim'))
sys.path.insert(0, os.environ['MATE_REFERENCE'])

import gym  # noqa: E402,F401  (the shim)
import mate  # noqa: E402  (the reference, read-only)

# one trace per entity shape among the recorded ones
TRACES = ('trace_1v1-9_greedy_s7', 'trace_2v2-9_random_s6', 'trace_2v4-0_greedy_s5', 'trace_4v2-9_random_s0', 'trace_4v8-0_random_s0',
          'trace_4v8-9_random_s0', 'trace_8v8-9_random_s0', 'trace_nav_random_s0')
MAX_STEPS = 64


def main():
    out = {'traces': np.array(TRACES)}
    for name in TRACES:
        fx = dict(np.load(os.path.join(HERE, name + '.npz')))
        env = mate.make('MultiAgentTracking-v0', config=str(fx['config_file']))
        space = env.state_space
        assert space.shape == fx['reset/state'].shape, (name, space.shape)
        steps = fx['step/state'][:MAX_STEPS]
        for rows in (fx['reset/state'][None], steps):      # the recorded states lie inside the box: the normalised rows are finite
            assert np.all(rows >= space.low) and np.all(rows <= space.high), name
        out[name + '/low'] = np.asarray(space.low, dtype=np.float64)
        out[name + '/high'] = np.asarray(space.high, dtype=np.float64)
        out[name + '/reset'] = mate.normalize_observation(fx['reset/state'].astype(np.float64), space)
        out[name + '/step'] = mate.normalize_observation(steps.astype(np.float64), space)
        assert np.all(np.isfinite(out[name + '/reset'])) and np.all(np.isfinite(out[name + '/step'])), name
    path = os.path.join(HERE, 'state_norm.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
