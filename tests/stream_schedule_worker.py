"""Worker of tests/test_stream_schedule_gpu.py::test_gatherer_stream_in_a_one_rank_group: a process of its own, because
dist.DetectionGatherer's communication stream exists only under an initialised RCCL process group (and the launcher
sets the environment RCCL needs before the HIP runtime starts).  One rank, 'nccl' backend, a file store: the G scenario
of the GPU file under every delay.  argv: <store file> <report json>.  Exit status 0 = every delayed run equalled the
plain run."""
import json
import os
import sys

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    store, report = sys.argv[1], sys.argv[2]
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    dist.init_process_group('nccl', init_method='file://' + store, rank=0, world_size=1, device_id=dev)
    try:
        import test_stream_schedule_gpu as t
        import guard_memory as gm
        sc = t.GatherScenario(dev)
        assert all(gm.same_bits(r['gathered'], r['records']) for r in sc.plain), 'one rank: the gather is a copy'
        outcome = t.all_delayed_runs_equal(sc)
        with open(report, 'w') as f:
            json.dump(dict(t.REPORT[sc.name], **outcome), f)
        print(f'{sc.name}: {outcome}', flush=True)
    finally:
        dist.destroy_process_group()


if __name__ == '__main__':
    main()
