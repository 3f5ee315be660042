"""Time EpidPipeline.run and its stages on 256 bench frames (`bench`), on their full-range stretch of bench.py's "#2w" (`wide`)
or on a flood field whose 400 mm cover the panel, so that no cell lies below the threshold (`flood`):
    python scripts/time_epid_step.py <bench|wide|flood> [reps]"""
import sys

import torch

sys.path.insert(0, ".")
from pylinac_amd.pipeline import EpidPipeline  # noqa: E402
from pylinac_amd.synthetic import epid_open_field_frames  # noqa: E402

mode = sys.argv[1]
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
dev = torch.device("cuda:0")
n = 256
fr = epid_open_field_frames(n, 1024, 1024, seed0=1000, device=dev, field_mm=400.0 if mode == "flood" else 200.0)
if mode == "wide":
    q = torch.quantile(fr[0].to(torch.float32).flatten()[::16], torch.tensor([0.01, 0.99], device=dev))
    lo_q, hi_q = float(q[0]), float(q[1])
    wide = torch.empty_like(fr)
    for a in range(0, n, 32):
        blk = ((fr[a:a + 32].to(torch.float32) - lo_q) * (64500.0 / (hi_q - lo_q)) + 500.0).round().clamp(0, 65535)
        wide.view(torch.int16)[a:a + 32] = blk.to(torch.int32).bitwise_and_(0xFFFF).to(torch.int16)
    fr = wide
pipe = EpidPipeline(n, 1024, 1024, dev)
for _ in range(10):
    res = pipe.run(fr)
torch.cuda.synchronize()
for rep in range(reps):
    ev = {}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(20):
        res = pipe.run(fr)
    e1.record()
    torch.cuda.synchronize()
    for _ in range(5):
        pipe.run(fr, ev)
    torch.cuda.synchronize()
    st = {k: round(sum(a.elapsed_time(b) for a, b in v) / len(v), 4) for k, v in ev.items()}
    print(f"{mode} ms_per_step={e0.elapsed_time(e1) / 20:.4f} stage_ms={st} flagged={int(pipe.flag.sum())} "
          f"zero_share={float((res.frames == 0).float().mean()):.4f}", flush=True)
