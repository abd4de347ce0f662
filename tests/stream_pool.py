"""Leave torch's stream pool where a test module found it (test infrastructure; a helper module, not a conftest).

torch.cuda.Stream() hands out the 32 streams of a per-device pool in turn, and the HIP runtime maps each of them onto
one of a few hardware queues.  Which pool stream - and so which hardware queue - a LATER test's side stream gets
therefore depends on how many streams every earlier test of the process took.  tests/test_stream_schedule_gpu.py
observes host-side waits that depend on that mapping (a blocking copy on the null stream queues behind a delay kernel
only when both share a hardware queue), so a new test module that takes streams - its own, or those of a model it
builds - would change what that file sees.  A module that uses `keep_pool_position` takes, when it is done, as many
further streams as complete a whole turn of the pool: every later torch.cuda.Stream() returns the stream it would have
returned had the module not run.
"""
import pytest

import stream_schedule as ss

POOL = 32       # c10's kStreamsPerPool


@pytest.fixture(scope='module', autouse=True)
def keep_pool_position():
    import torch
    with ss.recording_streams() as created:
        yield
        taken = len(created)
    for _ in range(-taken % POOL):
        torch.cuda.Stream(device=created[0].device)
