"""Time EpidPipeline.run and its stages on 256 frames of 1024 x 1024, one input pattern per run:
    bench   the bench frames, the same batch every step
    wide    their full-range stretch of bench.py's "#2w"
    flood   a flood field whose 400 mm cover the panel, so that no cell lies below the threshold
    alt     two batches of bench frames (seed0 1000 and 5000: centres up to +-5 px apart) take alternate steps
    worst   a bench batch and a flood batch take alternate steps: every cell that is below was stored non-zero the step before
python scripts/time_epid_step.py <pattern> [reps] [keep_zeros: 1|0]
`below` = share of cells under the threshold, `flip` = share of cells whose kept-zero entry differs between the two batches.
With two batches the stage times are per batch: "stage/0" = with the first batch named above as input, "stage/1" the second."""
import sys

import torch

sys.path.insert(0, ".")
from pylinac_amd.pipeline import EpidPipeline  # noqa: E402
from pylinac_amd.synthetic import epid_open_field_frames  # noqa: E402

mode = sys.argv[1]
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
keep = bool(int(sys.argv[3])) if len(sys.argv) > 3 else True
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
batches = [fr]
if mode == "alt":
    batches.append(epid_open_field_frames(n, 1024, 1024, seed0=5000, device=dev))
if mode == "worst":
    batches.append(epid_open_field_frames(n, 1024, 1024, seed0=1000, device=dev, field_mm=400.0))
pipe = EpidPipeline(n, 1024, 1024, dev, keep_zeros=keep)
step = 0


def run(events=None):
    global step
    res = pipe.run(batches[step % len(batches)], events)
    step += 1
    return res


def below():
    return pipe.cellmax.to(torch.int32) < pipe.thr[:, None, None]


for _ in range(10):
    res = run()
torch.cuda.synchronize()
flip = 0.0
if len(batches) > 1:
    before = below()
    run()
    flip = float((before != below()).float().mean())
    run()
for rep in range(reps):
    ev = {}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(20):
        res = run()
    e1.record()
    torch.cuda.synchronize()
    nb, first = len(batches), step
    for _ in range(5 if nb == 1 else 6):
        run(ev)
    torch.cuda.synchronize()
    # one batch: the average of the 5 runs; two: "stage/i" = that stage in the 3 runs whose input was batches[i]
    st = {}
    for k, v in ev.items():
        for i in range(nb):
            mine = v[(i - first) % nb::nb]
            st[k + (f"/{i}" if nb > 1 else "")] = round(sum(a.elapsed_time(b) for a, b in mine) / len(mine), 4)
    print(f"{mode} keep_zeros={int(keep)} ms_per_step={e0.elapsed_time(e1) / 20:.4f} stage_ms={st} flagged={int(pipe.flag.sum())} "
          f"zero_share={float((res.frames == 0).float().mean()):.4f} below={float(below().float().mean()):.4f} "
          f"flip={flip:.4f}", flush=True)
