"""Development aid: the EPID step with its three tails on one box -- the five launches, the colparts tail (one launch behind the
threshold launch) and the tail inside the threshold launch.  `python scripts/time_epid_tail.py [frames ...]` (default 256);
frames are 1024 x 1024;
a step = EpidPipeline.run + EpidResult.record(), what bench.py times."""
import sys
import time

import torch

sys.path.insert(0, ".")
from pylinac_amd.pipeline import EpidPipeline  # noqa: E402
from pylinac_amd.synthetic import epid_open_field_frames  # noqa: E402

dev = torch.device("cuda:0")
h, w = 1024, 1024
TAILS = (("separate", "five launches"), ("colparts", "colparts tail"), ("in_launch", "tail in launch"))
for n in [int(a) for a in sys.argv[1:]] or [256]:
    fr = epid_open_field_frames(n, h, w, seed0=1000, device=dev)
    pipes = {t: EpidPipeline(n, h, w, dev, tail=t) for t, _ in TAILS}

    def snapshot(res):
        return [getattr(res, k).cpu() for k in ("frames", "profile", "threshold", "status")] + [
            torch.nan_to_num(res.fwxm.cpu(), nan=-1), torch.nan_to_num(res.record().cpu(), nan=-1)]

    want = snapshot(pipes["separate"].run(fr))
    same = all(all(torch.equal(a, b) for a, b in zip(want, snapshot(pipes[t].run(fr)))) for t in ("colparts", "in_launch"))
    print(f"{n} frames: identical results: {same}", flush=True)
    for rep in range(3):
        for t, label in TAILS:
            p = pipes[t]
            for _ in range(20):
                p.run(fr).record()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(100):
                p.run(fr).record()
            torch.cuda.synchronize()
            print(n, "frames", label, round((time.perf_counter() - t0) * 10, 4), "ms per step", flush=True)
    del pipes, fr
    torch.cuda.empty_cache()
