#!/usr/bin/env python3
"""bench.py -- segmented patches/sec (448x448x3) on MI355X for the do_prediction hot path.

A *step* is one pass of the fused hot path over one batch of synthetic pages resident in HBM:
u8 page -> LUT normalise + tiling -> ResNet-50-U-Net forward (HIP, MFMA) -> softmax/argmax ->
margin-crop stitch -> u8 label map in HBM, page after page.

N = 1 (default): BASELINE.json configs[1] -- 3500x2500 pages, textline model (2 classes), margin 0.1 -> 70 tiles
of 448x448 per page; a step is `--pages-per-step` (32) such pages back to back, so that the timed region lasts
seconds, not a fraction of one (the clocks settle).  value = tiles / time over one timed region of exactly K steps
(`--steps`) after W warm-up steps (`--warmup`); `--repeats R` times R such regions and reports their median (all
repeats are listed; `--full` defaults to 3).

Plain run vs `--full`.  A plain `bench.py --gpus 1 --steps K --warmup W` does only what the headline needs: set up, warm
up, time the K steps, write `--dump-outputs DIR` if given, print the line.  Every side measurement and check -- the
roofline pass, the CPU baseline, the other arithmetic mode and the label check against the fp32 oracle, the host-memory
path, the one-page / pipeline3 / batch64 side workloads, the N > 1 exchange and per-rank figures -- runs with `--full`
only (and its `--no-*` switches trim it); the keys they fill are null otherwise.

`--dump-outputs DIR`: after the timed steps, the label maps the last step wrote (what a caller of the path receives) go to
DIR as .npy files (`dump_outputs`: the first page whole, a seeded sample of every page, per-page label counts; float32 /
float64, at most 64 MB).  Inputs are seeded: the same arguments give the same inputs on every run and build.

N > 1 (round 4: like for like with N = 1): the SAME page workload on every rank -- 16 such pages per GPU per step -- plus one RCCL
all-gather of the u8 masks per step (the "stitch" exchange north_star names); `scaling` = "weak" at every N, so value(N) / value(1)
is a scaling efficiency of one workload.  BASELINE.json configs[3] -- 64 pages of 4000x3000 (108 tiles each) sharded as whole pages
over the ranks, one all-gather of the masks per step, strong scaling -- is measured in the same run at EVERY N (N = 1 included:
the base of its curve) and reported under `batch64`; `--workload batch64` makes it the headline instead.
`SBBSEG_BENCH_COLLECTIVE=capi` routes the all-gather through the C ABI's own RCCL communicator (sbbseg_comm_* /
sbbseg_allgather_labels_dev: the path an integrator without torch uses) instead of torch.distributed.
One rank per GPU: either launched by
`python -m torch.distributed.run --nproc-per-node N bench.py --gpus N ...` (RANK / LOCAL_RANK / WORLD_SIZE in the
environment) or as plain `python bench.py --gpus N`, which re-executes itself under torch.distributed.run on
127.0.0.1 and relays the ranks' output.  The N > 1 line carries `ranks_seen` (world size and device of every rank, read
inside the process group), `exchange` (all-gather ms, algbw / busbw GB/s) and `per_rank` (each rank's rate on its own
shard with no collective).  NO multi-GPU curve has been measured by the builder: the build pool has 1-GPU boxes only.

Arithmetic modes.  `value` is the mode `--precision` names -- by default "f16x3", the label-exact split-fp16 mode
(hi + lo operands, three MFMAs per product; the default of the Python seams): it is the mode whose labels meet
north_star's "argmax label map bit-exact" bar against the fp32 oracle.  The fast plain-fp16 mode ("f16", BASELINE
configs[4]) is measured in the same run and reported under `modes` with its own roofline and label agreement.

Prints ONE JSON line on rank 0.  Extra objects with `--full`: `roofline` (dominant conv launch, HIP-event timed per launch
on the library's stream) and `cpu_baseline` (torch-CPU fp32 proxy of the Keras/TF CPU path on the host cores;
the oracle port is kept beside it), rank 0, N = 1.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

MFMA_PEAK_TFLOPS = 2500.0      # dense bf16/f16 MFMA, /opt/skills/guides/MI355X_MICROARCH.md
PAGE_H, PAGE_W = 3500, 2500    # BASELINE.json configs[1]
if os.environ.get("SBBSEG_BENCH_PAGE"):      # experiment knob (A/B of chunk sizes): "HxW" of the page workload's pages
    PAGE_H, PAGE_W = (int(v) for v in os.environ["SBBSEG_BENCH_PAGE"].lower().split("x"))
MODEL_HW, CLASSES = 448, 2
# committed rocprofv3 PMC summaries (tools/pmc_run.sh + tools/pmc_report.py) the `roofline.traffic` figure is read from: STATIC
# numbers (counters need their own profiling passes), valid only for the kernel sources they were collected on (csrc_sha)
PMC_SUMMARY = {"f16x3": os.path.join(ROOT, "profiles", "r06_x3_pmc_summary.json"),
               "f16": os.path.join(ROOT, "profiles", "r06_f16_pmc_summary.json")}


def csrc_sha():
    """Hash of the device / host sources libsbbseg is built from: ties a committed PMC summary to the kernels it measured."""
    import hashlib
    h = hashlib.sha1()
    for name in ("kernels.hip", "block_x3.hip", "stem_pool_x3.hip", "dec_halo_x3.hip", "dec_halo_f16.hip", "expand_reduce_x3.hip", "conv3_expand_reduce.hip", "region.hip", "region.h",
                 "api.hip", "internal.h"):
        with open(os.path.join(ROOT, "sbb_textline_detection_amd", "csrc", name), "rb") as f:
            h.update(f.read())
    return h.hexdigest()[:12]


DUMP_BUDGET_BYTES = 64 * 10 ** 6
DUMP_SAMPLE = 1 << 20


def dump_outputs(out_dir, outputs, seed=0):
    """`--dump-outputs`: write what the timed path's last step left in its output buffers, at most DUMP_BUDGET_BYTES in all.
    `outputs` = {name: uint8 label tensor [pages, H, W] or [H, W]}.  Per output: `<name>_counts` (float64 [pages, labels]: every
    page's label histogram), `<name>_sample` (float32: the labels at DUMP_SAMPLE flat positions of the whole tensor, drawn with
    numpy PCG64(seed) and sorted) with `<name>_sample_index` (float64: those positions), then, while the budget allows,
    `<name>_page0` (float32 [H, W]: the first page whole).  Returns the file names written."""
    import torch
    os.makedirs(out_dir, exist_ok=True)
    left, written, pages = DUMP_BUDGET_BYTES, [], []

    def save(name, arr):
        nonlocal left
        np.save(os.path.join(out_dir, name + ".npy"), arr)
        left -= arr.nbytes + 128                                    # + the .npy header
        written.append(name + ".npy")

    for name, t in outputs.items():
        t = t.reshape(-1, t.shape[-2], t.shape[-1])
        flat = t.reshape(-1)
        idx = np.sort(np.random.Generator(np.random.PCG64(seed)).integers(0, flat.numel(), min(DUMP_SAMPLE, flat.numel())))
        n_labels = int(t.max()) + 1
        save(name + "_counts", torch.stack([torch.bincount(p.reshape(-1), minlength=n_labels) for p in t]).cpu().numpy().astype(np.float64))
        save(name + "_sample", flat[torch.from_numpy(idx).to(flat.device)].cpu().numpy().astype(np.float32))
        save(name + "_sample_index", idx.astype(np.float64))
        pages.append((name, t[0]))
    for name, p in pages:
        if p.numel() * 4 + 128 <= left:
            save(name + "_page0", p.cpu().numpy().astype(np.float32))
    return written


def _free_port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _self_launch(n):
    """`python bench.py --gpus N` without a launcher: re-execute under torch.distributed.run, one rank per GPU, rendezvous on
    127.0.0.1, and relay the ranks' output (rank 0 prints the JSON line).  Returns the launcher's exit code."""
    import subprocess
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("OMP_NUM_THREADS", "8")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.call(cmd, env=env)


def _ranks_seen(dist, world, rank, local_rank, device_name):
    """What the process group itself reports: world size and (rank, local rank, device) of every member."""
    mine = {"rank": rank, "local_rank": local_rank, "device": device_name, "pid": os.getpid()}
    everyone = [None] * world
    dist.all_gather_object(everyone, mine)
    return {"world_size": dist.get_world_size(), "backend": dist.get_backend(), "ranks": everyone}


def _collective_choice():
    """SBBSEG_BENCH_COLLECTIVE: "torch" (default: torch.distributed all_gather_into_tensor, backend nccl = RCCL) or "capi" (the
    all-gather inside the C ABI: sbbseg_comm_init + sbbseg_allgather_labels_dev on the handle's stream, librccl dlopen'ed)."""
    v = os.environ.get("SBBSEG_BENCH_COLLECTIVE", "torch").lower()
    if v not in ("torch", "capi"):
        raise SystemExit(f"SBBSEG_BENCH_COLLECTIVE={v}: expected 'torch' or 'capi'")
    return v


def _default_workload(world):
    """`--workload auto`: the page workload (BASELINE configs[1]) at EVERY N, so that the driver's 1/2/4/8 sweep compares one
    workload with itself (weak scaling); configs[3] rides along under `batch64` at every N."""
    return "page"


def _broadcast_unique_id(dist, rank, make):
    """Rank 0 makes the 128-byte RCCL communicator id (`make()`), every rank returns the same bytes (shipped over the process group
    that torchrun's rendezvous built -- an integrator without torch ships them over its own channel)."""
    box = [make() if rank == 0 else None]
    dist.broadcast_object_list(box, src=0)
    return bytes(box[0])


def _plumbing_check(args):
    """Launch + rendezvous + collective only (no GPU, no model): gloo on CPU.  Exercised by the CPU tests at world 2 and 4 so
    that the round-end multi-GPU run cannot die in argument / launcher / process-group plumbing."""
    import torch
    import torch.distributed as dist
    world, rank, local_rank = int(os.environ["WORLD_SIZE"]), int(os.environ["RANK"]), int(os.environ.get("LOCAL_RANK", "0"))
    dist.init_process_group("gloo")
    seen = _ranks_seen(dist, world, rank, local_rank, "cpu")
    from sbb_textline_detection_amd.distributed import shard_block
    first, count, block = shard_block(64, rank, world)
    mine = torch.full((block, 4), rank, dtype=torch.uint8)
    everything = torch.empty((world * block, 4), dtype=torch.uint8)
    dist.all_gather_into_tensor(everything.view(-1), mine.view(-1))
    ok = all(int(everything[r * block, 0]) == r for r in range(world))
    # SBBSEG_BENCH_COLLECTIVE=capi: rank 0's 128-byte communicator id must reach every rank unchanged (here a stand-in id: the real
    # one needs RCCL and a GPU); every rank reports the digest of what it received
    collective = _collective_choice()
    uid_ok = None
    if collective == "capi":
        import hashlib
        uid = _broadcast_unique_id(dist, rank, lambda: bytes((7 * k + 1) & 0xFF for k in range(128)))
        digests = [None] * world
        dist.all_gather_object(digests, hashlib.sha1(uid).hexdigest())
        uid_ok = len(uid) == 128 and len(set(digests)) == 1
        ok = ok and uid_ok
    dist.barrier()
    if rank == 0:
        print(json.dumps({"plumbing_check": True, "n_gpus": world, "ranks_seen": seen, "all_gather_ok": ok, "collective": collective,
                          "unique_id_broadcast_ok": uid_ok, "default_workload": _default_workload(world),
                          "pages_per_rank": [shard_block(64, r, world)[1] for r in range(world)]}))
    dist.destroy_process_group()
    return 0 if ok else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=None,
                    help="timed regions of exactly --steps steps each; value = their median (default 1; 3 with --full)")
    ap.add_argument("--full", action="store_true",
                    help="also run every side measurement and check (roofline, CPU baseline, second mode + label check, host path, "
                         "side workloads, N > 1 exchange); a plain run times the headline only")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the label maps of the last timed step to DIR/<name>.npy (see dump_outputs)")
    ap.add_argument("--precision", default=os.environ.get("SBBSEG_BENCH_PRECISION", "f16x3"), choices=["f16", "bf16", "f16x3"],
                    help="arithmetic mode of `value`: f16x3 = label-exact split-fp16 (default), f16 = fast plain fp16")
    ap.add_argument("--max-batch", type=int, default=int(os.environ.get("SBBSEG_MAX_BATCH", "0")),
                    help="tiles per chunk (0 = 320 for the 3500x2500 pages -- two lanes of 160 --, 216 / 432 for the 4000x3000 pages of batch64)")
    ap.add_argument("--conv-variant", type=int, default=int(os.environ.get("SBBSEG_CONV_VARIANT", "0")),
                    help="A/B knob of the conv kernel (see sbbseg.h sbbseg_debug_set_conv_variant)")
    ap.add_argument("--workload", default="auto", choices=["auto", "page", "pipeline3", "batch64"],
                    help="auto = page at every N (BASELINE configs[1], the metric's config; weak scaling), with configs[3] (64 pages of "
                         "4000x3000 sharded over the ranks, strong scaling) measured beside it under `batch64` by --full; batch64 = configs[3] as the "
                         "headline; pipeline3 = configs[2] (border + layout + textline)")
    ap.add_argument("--pages-per-step", type=int, default=32, help="page workload: pages segmented back to back per step (32 x 70 tiles = 7 chunks of 320)")
    ap.add_argument("--batch-pages", type=int, default=64, help="batch64 workload: pages in the batch (64 = BASELINE configs[3])")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full: skip the CPU baseline (and with it the label check)")
    ap.add_argument("--no-second-mode", action="store_true", help="--full: skip the other arithmetic mode and the host-memory path")
    ap.add_argument("--no-extras", action="store_true", help="--full: skip the one-page, pipeline3 and batch64 side measurements")
    ap.add_argument("--cpu-patches", type=int, default=8, help="--full: tiles sampled for the CPU baseline and the label check")
    ap.add_argument("--plumbing-check", action="store_true",
                    help="launcher / rendezvous / all-gather only, gloo on CPU, no model (CPU tests of the N > 1 launch path)")
    args = ap.parse_args()
    if args.repeats is None:
        args.repeats = 3 if args.full else 1

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        raise SystemExit(_self_launch(args.gpus))           # plain `python bench.py --gpus N`: become the launcher
    if "WORLD_SIZE" in os.environ and int(os.environ["WORLD_SIZE"]) != args.gpus:
        raise SystemExit(f"WORLD_SIZE={os.environ['WORLD_SIZE']} but --gpus {args.gpus}")
    if args.plumbing_check:
        if "WORLD_SIZE" not in os.environ:                  # --gpus 1: a world of one
            os.environ.update(WORLD_SIZE="1", RANK="0", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()))
        raise SystemExit(_plumbing_check(args))

    import torch
    import torch.distributed as dist

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit(f"WORLD_SIZE={world} but --gpus {args.gpus}")
    # SBBSEG_BENCH_BACKEND=gloo: the N > 1 code path on a box with fewer GPUs than ranks (ranks share devices, the all-gather
    # is staged through host memory) -- a functional check of the sharded workload, never a scaling number
    backend = os.environ.get("SBBSEG_BENCH_BACKEND", "nccl")
    n_dev = torch.cuda.device_count()
    if n_dev < 1:
        raise SystemExit("bench.py needs a GPU: the HIP path has no CPU fallback")
    if backend == "nccl" and world > n_dev:
        raise SystemExit(f"--gpus {world} but only {n_dev} GPU(s) visible (RCCL needs one device per rank)")
    device_index = local_rank % n_dev
    workload = args.workload if args.workload != "auto" else _default_workload(world)
    collective = _collective_choice()
    if collective == "capi" and backend != "nccl":
        raise SystemExit("SBBSEG_BENCH_COLLECTIVE=capi needs one GPU per rank (RCCL): not available under the gloo check backend")
    if args.max_batch <= 0:
        # tiles per chunk: four pages' worth (4 x 70 / 4 x 108), pooled across pages by sbbseg_segment_pages_dev and run as two
        # concurrent halves -- one page's 70 tiles leave the persistent conv grids a ragged last round; 140 / 280 / 374 / 560
        # tiles per chunk measured 9 997 / 10 176 / 10 214 / 10 209 patches/s (profiles/r02_experiments.md)
        # (f16x3 stores 4 bytes per activation element: a tensor x batch must stay inside the 4 GiB gather window -- the largest,
        # 224x224x64, allows 334 patches -- so the 4000x3000 pages pool two at a time there, 2 x 108 tiles)
        # Round 5: 320 tiles per chunk = 160 per lane.  The persistent conv grids walk their tiles in rounds of 256 blocks; a lane batch
        # of 160 patches gives the long launches 3.84 / 7.66 / 15.3 / 1.91 / 0.96 rounds (dec1 / dec2 / dec3 / the stage-4 and stage-5
        # 3x3 convs: 160 x 196 px = 122.5 tiles of 256 px) where 140 gave 3.375 / 6.7 / 13.4 / 1.68 / 0.84 -- the last round of every such
        # launch ran 37-84 % full.  (166 would fill them to 99 %; the fast gather's 2^31-byte window on the 224 x 224 x 64 tensor stops
        # at 167 patches per launch.)  A step is 32 pages = 2 240 tiles = 7 chunks.
        args.max_batch = (216 if args.precision == "f16x3" else 432) if workload == "batch64" else (320 if workload == "page" else 70)
    torch.cuda.set_device(device_index)
    ranks_seen = None
    if world > 1:
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", device_index))
        else:
            dist.init_process_group(backend)
        ranks_seen = _ranks_seen(dist, world, rank, local_rank, torch.cuda.get_device_name(device_index))

    comm_state = {"ctx": None}

    def all_gather_u8(dst, src_t):
        """the stitch exchange: every rank's u8 masks to every rank (RCCL; host-staged under the gloo check backend)"""
        if collective == "capi":
            # ncclAllGather on the handle's stream (= torch's current stream here), communicator owned by the library
            comm_state["ctx"].allgather_labels_dev(src_t.data_ptr(), src_t.numel(), dst.data_ptr())
        elif backend == "nccl":
            dist.all_gather_into_tensor(dst.view(-1), src_t.view(-1))
        else:
            h = torch.empty(dst.numel(), dtype=torch.uint8)
            dist.all_gather_into_tensor(h, src_t.view(-1).cpu())
            dst.view(-1).copy_(h)

    from sbb_textline_detection_amd import _capi
    from sbb_textline_detection_amd.model import SegModel
    from sbb_textline_detection_amd.synthetic import synthetic_page
    from tools.synth_model import calibrated_model

    cfg, weights = calibrated_model(CLASSES, MODEL_HW, MODEL_HW, seed=0)
    stream = torch.cuda.current_stream().cuda_stream

    def make_model(precision, classes_cfg=None, max_batch=None):
        c, w = classes_cfg or (cfg, weights)
        m = SegModel(c, w, device=device_index, max_batch=max_batch or args.max_batch, precision=precision)
        m.ctx.set_stream(stream)
        m.ctx.set_conv_variant(args.conv_variant)
        return m

    model = make_model(args.precision)
    if world > 1 and collective == "capi":
        uid = _broadcast_unique_id(dist, rank, _capi.comm_unique_id)
        model.ctx.comm_init(rank, world, uid)
        if model.ctx.comm_info() != (rank, world):
            raise SystemExit("sbbseg_comm_init: communicator does not report (rank, world)")
        comm_state["ctx"] = model.ctx
    tiles_per_page = _capi.tile_grid(PAGE_H, PAGE_W, MODEL_HW, MODEL_HW)[0].shape[0]
    page0 = synthetic_page(PAGE_H, PAGE_W, seed=rank)

    fallbacks_of_pipeline3 = lambda: 0
    page_state = {}
    # ---- workloads: build(model) -> (step(), tiles per step, description, scaling, gather() or None, bytes gathered)
    def build_page(m):
        P = max(1, args.pages_per_step)
        # the pages are drawn on a few host threads (numpy's generators and array ops release the GIL for most of the work): one
        # 3500x2500 page costs a third of a second on one core, 32 of them serially would dwarf a short timed region
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(max_workers=max(1, min(16, P - 1, os.cpu_count() or 1))) as ex:
            drawn = ex.map(lambda k: synthetic_page(PAGE_H, PAGE_W, seed=rank * 1000 + k), range(1, P))
            pages = [torch.from_numpy(page0).cuda()] + [torch.from_numpy(p_).cuda() for p_ in drawn]
        labels = torch.empty((P, PAGE_H, PAGE_W), dtype=torch.uint8, device="cuda")
        d_all = torch.empty((world, P, PAGE_H, PAGE_W), dtype=torch.uint8, device="cuda") if world > 1 else None
        page_state[id(m)] = labels                  # the buffer the timed steps write: label_match reads it back afterwards

        def gather():
            all_gather_u8(d_all, labels)

        page_ptrs, label_ptrs = [p_.data_ptr() for p_ in pages], [labels[k].data_ptr() for k in range(P)]

        def step():
            m.ctx.segment_pages_dev(page_ptrs, PAGE_H, PAGE_W, label_ptrs)      # tiles pooled across pages, chunks of max_batch
            if world > 1:
                gather()
        desc = f"BASELINE configs[1] x {P}: {P} pages of {PAGE_H}x{PAGE_W} ({tiles_per_page} tiles of 448x448 each, margin 0.1) per GPU per step, textline model, {CLASSES} classes"
        def step_local():
            m.ctx.segment_pages_dev(page_ptrs, PAGE_H, PAGE_W, label_ptrs)
        step.ctxs = step_local.ctxs = [m.ctx]
        step.outputs = {"labels": labels}
        return step, tiles_per_page * P * world, desc, "weak", (gather if world > 1 else None), P * PAGE_H * PAGE_W * world, step_local, tiles_per_page * P

    def build_batch64(m, distinct=None):
        """`distinct`: how many different synthetic pages back the batch (None = every page its own seed); the side measurement of the
        default line cycles 8 (drawing 64 pages of 4000x3000 on one host core would cost more than the measurement itself)."""
        BH, BW, NPAGES = 4000, 3000, max(1, args.batch_pages)
        from sbb_textline_detection_amd.distributed import shard_block
        first, count, block = shard_block(NPAGES, rank, world)
        drawn = {}
        def page_of(k):
            key = (first + k) if distinct is None else (first + k) % distinct
            if key not in drawn:
                drawn[key] = torch.from_numpy(synthetic_page(BH, BW, seed=100 + key)).cuda()
            return drawn[key]
        pages = [page_of(k) for k in range(count)]
        d_mine = torch.empty((block, BH, BW), dtype=torch.uint8, device="cuda")
        d_everything = torch.empty((world * block, BH, BW), dtype=torch.uint8, device="cuda") if world > 1 else None
        tpp = _capi.tile_grid(BH, BW, MODEL_HW, MODEL_HW)[0].shape[0]

        def gather():
            all_gather_u8(d_everything, d_mine)

        page_ptrs, label_ptrs = [p_.data_ptr() for p_ in pages], [d_mine[k].data_ptr() for k in range(count)]

        def step():
            if count:
                m.ctx.segment_pages_dev(page_ptrs, BH, BW, label_ptrs)
            if world > 1:
                gather()
        desc = f"BASELINE configs[3]: {NPAGES} pages of {BH}x{BW} ({tpp} tiles each) sharded as whole pages over the ranks + one all-gather of the masks per step"
        def step_local():
            if count:
                m.ctx.segment_pages_dev(page_ptrs, BH, BW, label_ptrs)
        step.ctxs = step_local.ctxs = [m.ctx]
        step.outputs = {"labels": d_mine[:count]}
        return step, tpp * NPAGES, desc, "strong", (gather if world > 1 else None), world * block * BH * BW, step_local, tpp * count

    def build_pipeline3(m):
        """BASELINE configs[2] as textline_detector.run() chains it (main.py:2056-2107): get_image_and_scales (3500x2500 -> 4200x3000,
        fused into the gathers), border model on the whole page + page box, then the layout model (Otsu'd) and the textline model
        on the CROPPED page, text regions cleaned by erode x 3 / dilate x 4.  Models resident; the page starts in (pinned) host memory,
        is uploaded once per step and stays resident in HBM for all three stages (the border mask never leaves the device: in the
        reference it is a local of extract_page, only the box and the crop leave it)."""
        from sbb_textline_detection_amd.stages import scaled_size
        cfg_b, w_b = calibrated_model(2, MODEL_HW, MODEL_HW, seed=11)
        cfg_l, w_l = calibrated_model(4, MODEL_HW, MODEL_HW, seed=12)
        Hs, Ws = scaled_size(PAGE_H, PAGE_W)
        n_full = _capi.tile_grid(Hs, Ws, MODEL_HW, MODEL_HW)[0].shape[0]
        m_border = make_model(m.precision, (cfg_b, w_b), max_batch=1)
        m_layout = make_model(m.precision, (cfg_l, w_l), max_batch=n_full)
        m_text = make_model(m.precision, None, max_batch=n_full) if m.max_batch < n_full else m
        h_page = torch.from_numpy(page0).pin_memory()                              # the page starts in (pinned) host memory ...
        d_page = torch.empty_like(h_page, device="cuda")                            # ... and is uploaded ONCE per step, for all three stages
        d_page.copy_(h_page)
        box, pixels = m_border.ctx.extract_page_box_dev(d_page.data_ptr(), PAGE_H, PAGE_W, Hs, Ws)
        if pixels == 0 or box[2] < MODEL_HW or box[3] < MODEL_HW:
            box = (0, 0, Ws, Hs)                                                    # main.py:417-419: fall back to the whole page
        bw, bh = box[2], box[3]
        tiles_crop = _capi.tile_grid(bh, bw, MODEL_HW, MODEL_HW)[0].shape[0]
        d_regions = torch.empty((bh, bw), dtype=torch.uint8, device="cuda")
        d_clean = torch.empty((bh, bw), dtype=torch.uint8, device="cuda")
        d_lines = torch.empty((bh, bw), dtype=torch.uint8, device="cuda")

        c0 = m_border.ctx.host_contour_calls()
        nonlocal fallbacks_of_pipeline3
        fallbacks_of_pipeline3 = lambda: m_border.ctx.host_contour_calls() - c0      # how often the box needed the exact host ranking

        def step():
            d_page.copy_(h_page, non_blocking=True)                                 # H2D on the current stream = the handles' stream
            m_border.ctx.extract_page_box_dev(d_page.data_ptr(), PAGE_H, PAGE_W, Hs, Ws)      # border model + dilate x 6 + largest contour + box
            m_layout.ctx.segment_crop_dev(d_page.data_ptr(), PAGE_H, PAGE_W, Hs, Ws, box, True, d_regions.data_ptr())
            m_layout.ctx.morph_dev(d_regions.data_ptr(), bh, bw, 0, 5, 3, d_clean.data_ptr())      # main.py:2074-2075
            m_layout.ctx.morph_dev(d_clean.data_ptr(), bh, bw, 1, 5, 4, d_clean.data_ptr())
            m_text.ctx.segment_crop_dev(d_page.data_ptr(), PAGE_H, PAGE_W, Hs, Ws, box, False, d_lines.data_ptr())
        # the same calls one by one, for the breakdown printed beside the total (each timed alone, with a synchronize on both sides)
        step.stages = {
            "upload_ms": lambda: d_page.copy_(h_page, non_blocking=True),
            "border_forward_and_page_box_ms": lambda: m_border.ctx.extract_page_box_dev(d_page.data_ptr(), PAGE_H, PAGE_W, Hs, Ws),
            "layout_stage_ms": lambda: m_layout.ctx.segment_crop_dev(d_page.data_ptr(), PAGE_H, PAGE_W, Hs, Ws, box, True, d_regions.data_ptr()),
            "erode3_dilate4_ms": lambda: (m_layout.ctx.morph_dev(d_regions.data_ptr(), bh, bw, 0, 5, 3, d_clean.data_ptr()),
                                          m_layout.ctx.morph_dev(d_clean.data_ptr(), bh, bw, 1, 5, 4, d_clean.data_ptr())),
            "textline_stage_ms": lambda: m_text.ctx.segment_crop_dev(d_page.data_ptr(), PAGE_H, PAGE_W, Hs, Ws, box, False, d_lines.data_ptr()),
        }
        step.ctxs = [m_border.ctx, m_layout.ctx] + ([m_text.ctx] if m_text is not m_layout else [])
        step.outputs = {"text_regions": d_clean, "textlines": d_lines}
        desc = f"BASELINE configs[2]: border + layout + textline on one {PAGE_H}x{PAGE_W} page ({Hs}x{Ws} upscaled, box {box}, {tiles_crop} tiles per patch stage)"
        return step, (1 + 2 * tiles_crop) * world, desc, "weak", None, 0, None, 1 + 2 * tiles_crop

    builders = {"page": build_page, "batch64": build_batch64, "pipeline3": build_pipeline3}

    def fence():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    def timed(step, steps, warmup, repeats):
        for _ in range(warmup):
            step()
        out = []
        for _ in range(repeats):
            fence()
            t0 = time.perf_counter()
            for _ in range(steps):
                step()
            fence()
            dt = time.perf_counter() - t0
            if world > 1:
                t = torch.tensor([dt], dtype=torch.float64, device="cuda")
                dist.all_reduce(t, op=dist.ReduceOp.MAX)
                dt = float(t.item())
            out.append(dt)
        return out

    def forwards_of(step_fn, whole_job=True):
        """Forwards the handles REALLY run in one step (sbbseg_debug_counter 1 = patches through the plan), summed over the ranks.  The
        fused page paths compute a repeated clamped tile once (sbbseg_set_dedupe, default on): on page sizes with extent % 360 in (0, 88]
        this is less than the reference's call count (4000 x 3000: 99 forwards for 108 calls) -- rates are quoted on what ran."""
        before = forwards_now(step_fn)
        step_fn()
        torch.cuda.synchronize()
        n = forwards_now(step_fn) - before
        return summed_over_ranks(n) if whole_job else int(n)

    def forwards_now(step_fn):
        """the handles' forward counters (host-side: bumped as the calls enqueue work)"""
        return sum(c.forwards() for c in {id(c): c for c in step_fn.ctxs}.values())

    def summed_over_ranks(n):
        if world > 1:
            t = torch.tensor([n], dtype=torch.int64, device="cuda" if backend == "nccl" else "cpu")
            dist.all_reduce(t, op=dist.ReduceOp.SUM)
            n = int(t.item())
        return int(n)

    step, reference_calls_per_step, workload_desc, scaling, gather, gathered_bytes, step_local, local_calls = builders[workload](model)

    def executed_flops_per_patch(ctx):
        """FLOPs (reference formulation, per op) the handle EXECUTED per forward since its last profile_reset: owned-region launches
        (sbbseg_set_owned_regions) walk a part of a decoder level's output grid and count that share (sbbseg_op_executed)."""
        prof = ctx.profile()
        fw = max(o["exec_patches"] for o in prof)
        return sum(o["flops"] * o["exec_patches"] for o in prof) / fw if fw else 0.0
    model.ctx.profile_reset()
    before = forwards_now(step)
    dts = timed(step, args.steps, args.warmup, max(1, args.repeats))
    # what `value` counts: forwards executed per step, whole job, read off the counters over the warm-up and timed steps
    tiles_per_step = summed_over_ranks(forwards_now(step) - before) // (args.warmup + args.steps * max(1, args.repeats))
    exec_flops = executed_flops_per_patch(model.ctx) if workload != "pipeline3" else 2 * model.plan.macs_per_patch()
    dt = statistics.median(dts)
    value = tiles_per_step * args.steps / dt
    rates = [tiles_per_step * args.steps / t for t in dts]
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, step.outputs)
    # what the timed steps themselves wrote: page 0's mask out of the pooled label buffer, read back before any other call
    timed_labels0 = page_state[id(model)][0].cpu().numpy() if (args.full and rank == 0 and workload == "page") else None

    exchange, per_rank = None, None
    if gather is not None and args.full:                            # the exchange alone: all-gather GB/s over xGMI
        for _ in range(2):
            gather()
        fence()
        t0 = time.perf_counter()
        for _ in range(10):
            gather()
        fence()
        gdt = (time.perf_counter() - t0) / 10
        exchange = {"collective": "all_gather_into_tensor (RCCL)" if backend == "nccl" else f"host-staged all-gather ({backend})",
                    "bytes_gathered_per_rank": gathered_bytes,
                    "ms": round(gdt * 1e3, 3), "algbw_GBps": round(gathered_bytes / gdt / 1e9, 1),
                    "busbw_GBps": round(gathered_bytes * (world - 1) / world / gdt / 1e9, 1),
                    "share_of_step": round(gdt / (dt / args.steps), 4)}
        # every rank's rate on its own shard with NO collective and no barrier inside the loop (what the exchange and the
        # slowest-rank wait cost is value vs the sum of these)
        local_step = step_local if step_local is not None else step
        local_tiles = forwards_of(step_local, whole_job=False) if step_local is not None else tiles_per_step // world
        n_loc = max(2, args.steps // 4)
        fence()
        t0 = time.perf_counter()
        for _ in range(n_loc):
            local_step()
        torch.cuda.synchronize()
        mine = torch.tensor([local_tiles * n_loc / (time.perf_counter() - t0)], dtype=torch.float64, device="cuda")
        rates_all = [torch.zeros_like(mine) for _ in range(world)]
        if backend == "nccl":
            dist.all_gather(rates_all, mine)
        else:
            rl = [None] * world
            dist.all_gather_object(rl, float(mine.item()))
            rates_all = [torch.tensor([v]) for v in rl]
        pr = [round(float(t.item()), 1) for t in rates_all]
        per_rank = {"compute_only_patches_per_s": pr, "sum": round(sum(pr), 1)}      # each rank on its own shard, no all-gather, no barrier

    # ---- BASELINE configs[3] beside the headline, at EVERY N (N = 1 = the base of its strong-scaling curve) --------------
    batch64 = None
    if args.full and workload == "page" and not args.no_extras:
        try:
            stepb, callsb, descb, scalb, gatherb, bytesb = build_batch64(model, distinct=8)[:6]
            tilesb = forwards_of(stepb)                                 # forwards executed (4000 x 3000: 99 per page, the reference calls 108)
            nb = max(2, min(4, args.steps // 5))
            dtb = timed(stepb, nb, 0, 1)[0]
            batch64 = {"patches_per_s": round(tilesb * nb / dtb, 2), "ms_per_step": round(dtb / nb * 1e3, 3), "steps": nb, "warmup": 1,
                       "scaling": scalb, "tiles_per_step": tilesb, "forwards_per_step": tilesb, "reference_calls_per_step": callsb,
                       "dedupe": tilesb != callsb, "reference_calls_per_s": round(callsb * nb / dtb, 2),
                       "pages": max(1, args.batch_pages), "chunk_tiles": model.max_batch}
            if gatherb is not None:
                for _ in range(2):
                    gatherb()
                fence()
                t0 = time.perf_counter()
                for _ in range(5):
                    gatherb()
                fence()
                gdtb = (time.perf_counter() - t0) / 5
                batch64["exchange"] = {"bytes_gathered_per_rank": bytesb, "ms": round(gdtb * 1e3, 3),
                                       "algbw_GBps": round(bytesb / gdtb / 1e9, 1),
                                       "busbw_GBps": round(bytesb * (world - 1) / world / gdtb / 1e9, 1),
                                       "share_of_step": round(gdtb / (dtb / nb), 4)}
            del stepb, gatherb
            torch.cuda.empty_cache()
        except Exception as e:                                          # never lose the headline over the side measurement
            batch64 = {"error": repr(e)}

    # ---- roofline of the dominant kernel: per-launch HIP events on the library's stream ----------
    def roofline_of(m):
        d_page = torch.from_numpy(page0).cuda()
        d_labels = torch.empty((PAGE_H, PAGE_W), dtype=torch.uint8, device="cuda")
        c = m.ctx
        c.profile_enable(True)
        c.profile_reset()
        # (profiling runs every launch alone on one lane, in LANE-sized launches: chunks of max_batch / 2 tiles pooled across pages -- the
        # launches the timed region's two lanes run; 16 pages = 1 120 tiles = 7 launches of 160 per op at the default max_batch of 320)
        d_page2 = torch.from_numpy(synthetic_page(PAGE_H, PAGE_W, seed=4242)).cuda()
        n_prof_pages = 16
        d_labels_prof = torch.empty((n_prof_pages, PAGE_H, PAGE_W), dtype=torch.uint8, device="cuda")
        prof_pages = [(d_page if k % 2 == 0 else d_page2).data_ptr() for k in range(n_prof_pages)]
        for _ in range(2):
            c.segment_pages_dev(prof_pages, PAGE_H, PAGE_W, [d_labels_prof[k].data_ptr() for k in range(n_prof_pages)])
        torch.cuda.synchronize()
        del d_labels
        prof = c.profile()
        c.profile_enable(False)
        convs = [o for o in prof if ("conv" in o["name"] or o["name"].startswith("block")) and o["launches"] > 0]       # incl. stem_conv*, direct_conv*, tail_conv*, fused bottleneck blocks
        tot_ms = sum(o["total_ms"] for o in prof)

        # every rate is priced on EXECUTED work: an owned-region launch counts the share of the output grid it walked
        # (timed_exec_patches = whole-patch equivalents over the launches total_ms covers), so a fraction cannot rise because work disappeared
        def rate(ops, key="flops"):
            ms = sum(o["total_ms"] for o in ops)
            return sum(o[key] * o["timed_exec_patches"] for o in ops) / (ms * 1e-3) / 1e12 if ms else 0.0
        def rate_all(key="flops"):
            # ALL convs of the plan over the time of the launches that run them (an op fused into another op's launch has launches == 0)
            every = [o for o in prof if ("conv" in o["name"] or o["name"].startswith("block"))]
            ms = sum(o["total_ms"] for o in every)
            return sum(o[key] * o["timed_exec_patches"] for o in every) / (ms * 1e-3) / 1e12 if ms else 0.0
        # the three 3x3 convs of stage 2 run inside the fused block launches (block_*_HxW): their FLOPs (2 x 9 x 64 x 64 x H x W) with the
        # share of the block's time that their share of its FLOPs is
        def stage2_3x3():
            fl = ms = iss = 0.0
            for o in prof:
                if o["name"].startswith("block") and o["launches"] > 0 and o["flops"] > 0:
                    hh, ww = (int(v) for v in o["name"].rsplit("_", 1)[1].split("x"))
                    f3 = 2.0 * 9 * 64 * 64 * hh * ww
                    share = f3 / o["flops"]
                    fl += f3 * o["timed_exec_patches"]; iss += o["issued_flops"] * share * o["timed_exec_patches"]; ms += o["total_ms"] * share
            return fl, iss, ms
        # an op that launches nothing of its own (its events bracket ~5 us of host time) is computed inside a neighbour's launch: the
        # reduce conv behind an expand (expand_reduce), and since round 6 the 3x3 conv in FRONT of a stage-3 expand (conv3_expand_reduce)
        def riding(o):
            return o["launches"] > 0 and o["total_ms"] / o["launches"] < 0.02
        # the 3x3 convs riding in an expand's launch: their FLOPs with the share of that launch's time that their share of its issued FLOPs is
        def fused_3x3():
            fl = ms = iss = 0.0
            for i, o in enumerate(prof):
                if "conv3x3" in o["name"] and riding(o) and i + 1 < len(prof):
                    host = prof[i + 1]
                    group = [o, host] + ([prof[i + 2]] if i + 2 < len(prof) and riding(prof[i + 2]) else [])
                    share = o["issued_flops"] / sum(g["issued_flops"] for g in group)
                    fl += o["flops"] * o["timed_exec_patches"]; iss += o["issued_flops"] * o["timed_exec_patches"]; ms += host["total_ms"] * share
            return fl, iss, ms
        # dominant kernel launch = the conv launch with the largest average duration (the four output-
        # parity classes of a decoder conv run as one grouped launch)
        dom = max(convs, key=lambda o: o["total_ms"] / o["launches"])
        k3 = [o for o in convs if any(t in o["name"] for t in ("conv3x3", "conv2x2")) and not riding(o)]          # the 3x3 conv stages (their own launches)
        ach, iss = rate([dom]), rate([dom], "issued_flops")
        s2_fl, s2_iss, s2_ms = stage2_3x3()
        f3_fl, f3_iss, f3_ms = fused_3x3()
        k3_ms = sum(o["total_ms"] for o in k3)
        k3_fl = sum(o["flops"] * o["timed_exec_patches"] for o in k3)
        k3_iss = sum(o["issued_flops"] * o["timed_exec_patches"] for o in k3)
        # `conv3x3_stages` = the 3x3 convs with a launch of their own; `conv3x3_stages_incl_stage2` adds every 3x3 conv that runs inside
        # another launch -- the three of stage 2 (fused blocks) and the two of stage 3 that ride in conv3_expand_reduce -- with the share of
        # that launch's time that their share of its (issued) FLOPs is
        s2_fl, s2_iss, s2_ms = s2_fl + f3_fl, s2_iss + f3_iss, s2_ms + f3_ms
        # (what the numbers mean -- algorithmic vs issued vs executed FLOPs, the profiling pass, peak / 3 in the split mode -- is
        #  written up in DESIGN.md section 6: the line carries numbers only, so that the driver's record keeps all of it)
        r = {
            "bound": "mfma", "kernel": "conv_igemm_mfma:" + dom["name"],
            "achieved": round(ach, 2), "peak": MFMA_PEAK_TFLOPS, "unit": "TFLOP/s",
            "frac": round(ach / MFMA_PEAK_TFLOPS, 4),
            "achieved_issued": round(iss, 2), "frac_issued": round(iss / MFMA_PEAK_TFLOPS, 4),
            "traffic": None,
            "avg_launch_ms": round(dom["total_ms"] / dom["launches"], 4),
            "patches_per_launch": dom["patches"] / dom["launches"],
            "executed_share_of_launch": round(dom["timed_exec_patches"] / dom["patches"], 4),
            "flops_per_launch": dom["flops"] * dom["timed_exec_patches"] / dom["launches"],
            "issued_flops_per_launch": dom["issued_flops"] * dom["timed_exec_patches"] / dom["launches"],
            # the three longest conv launches (the reported kernel is the first): which one is longest changes as they are tuned
            "longest_launches": [{"name": o["name"], "avg_launch_ms": round(o["total_ms"] / o["launches"], 4),
                                  "frac": round(rate([o]) / MFMA_PEAK_TFLOPS, 4), "frac_issued": round(rate([o], "issued_flops") / MFMA_PEAK_TFLOPS, 4)}
                                 for o in sorted(convs, key=lambda o: -o["total_ms"] / o["launches"])[:3]],
            "conv3x3_stages": {"achieved": round(k3_fl / (k3_ms * 1e-3) / 1e12, 2) if k3_ms else 0.0,
                               "frac": round(k3_fl / (k3_ms * 1e-3) / 1e12 / MFMA_PEAK_TFLOPS, 4) if k3_ms else 0.0,
                               "frac_issued": round(k3_iss / (k3_ms * 1e-3) / 1e12 / MFMA_PEAK_TFLOPS, 4) if k3_ms else 0.0,
                               "share_of_gpu_time": round(k3_ms / tot_ms, 4)},
            # ... with the three stage-2 3x3 convs (inside the fused block launches) counted in
            "conv3x3_stages_incl_stage2": {"frac": round((k3_fl + s2_fl) / ((k3_ms + s2_ms) * 1e-3) / 1e12 / MFMA_PEAK_TFLOPS, 4) if k3_ms + s2_ms else 0.0,
                                           "frac_issued": round((k3_iss + s2_iss) / ((k3_ms + s2_ms) * 1e-3) / 1e12 / MFMA_PEAK_TFLOPS, 4) if k3_ms + s2_ms else 0.0,
                                           "share_of_gpu_time": round((k3_ms + s2_ms) / tot_ms, 4)},
            "all_convs": {"achieved": round(rate_all(), 2), "frac": round(rate_all() / MFMA_PEAK_TFLOPS, 4),
                          "frac_issued": round(rate_all("issued_flops") / MFMA_PEAK_TFLOPS, 4),
                          "share_of_gpu_time": round(sum(o["total_ms"] for o in convs) / tot_ms, 4)},
            "profiled_ms_per_lane_launch_set": round(tot_ms / max(1, dom["launches"]), 3),
        }
        if m.precision == "f16x3":
            # the split mode issues three f16 MFMAs per product: algorithmic work cannot exceed a third of the dense f16 peak
            r["frac_of_split_peak"] = round(ach / (MFMA_PEAK_TFLOPS / 3), 4)
        # HBM-side traffic of that launch from the committed rocprofv3 PMC passes of this same command (tools/pmc_run.sh;
        # counters need their own runs, see profiles/): bytes per launch.  STATIC: read from a file, not measured in this run;
        # dropped (null) when the file was collected on other kernel sources than the ones this library was built from.
        try:
            path = PMC_SUMMARY.get(m.precision)
            pmc = json.load(open(path)) if path and os.path.exists(path) else None
            if pmc is not None and pmc.get("csrc_sha") != csrc_sha():
                r["traffic_note"] = "PMC summary %s is stale (csrc %s, this build %s)" % (os.path.basename(path), pmc.get("csrc_sha"), csrc_sha())
                pmc = None
            ent = pmc["ops"].get(dom["name"]) if pmc is not None and pmc.get("precision", "f16") == m.precision else None
            if ent and abs(dom["patches"] / dom["launches"] - pmc.get("patches_per_launch", 70)) < 1e-6:
                r["traffic"] = round(ent["fetch_bytes"] + ent["write_bytes"])
                r["traffic_static"] = True
                if "mfma_busy_pct" in ent:
                    r["mfma_pipe_busy_pct_pmc"] = ent["mfma_busy_pct"]
                r["traffic_source"] = "STATIC: %s, csrc %s" % (os.path.relpath(path, ROOT), pmc.get("csrc_sha"))
        except Exception:
            pass
        per_op = [{"name": o["name"], "ms_per_launch": round(o["total_ms"] / o["launches"], 4), "patches_per_launch": o["patches"] / o["launches"],
                   "executed_share": round(o["timed_exec_patches"] / o["patches"], 4) if o["patches"] else 1.0,
                   "tflops": round(o["flops"] * o["timed_exec_patches"] / (o["total_ms"] * 1e-3) / 1e12, 1) if o["total_ms"] else 0,
                   "tflops_issued": round(o["issued_flops"] * o["timed_exec_patches"] / (o["total_ms"] * 1e-3) / 1e12, 1) if o["total_ms"] else 0}
                  for o in prof if o["launches"]]
        return r, per_op

    roofline, per_op = (roofline_of(model) if args.full and rank == 0 else (None, []))

    # ---- the same pages starting (and ending) in HOST memory: never `value`, reported beside it -------------------------
    host_path = None
    if args.full and rank == 0 and world == 1 and workload == "page" and not args.no_second_mode:
        hp_pages = [page0 if k == 0 else synthetic_page(PAGE_H, PAGE_W, seed=k) for k in range(max(1, args.pages_per_step))]
        model.ctx.segment_pages(hp_pages[:4])                                  # allocates the pinned staging
        t0 = time.perf_counter()
        for _ in range(2):
            model.ctx.segment_pages(hp_pages)
        t_pipe = (time.perf_counter() - t0) / 2
        t0 = time.perf_counter()
        for p_ in hp_pages:
            model.ctx.segment_page(p_)
        t_serial = time.perf_counter() - t0
        # numpy pages in host memory -> numpy label maps in host memory, PCIe both ways inside the time (sbbseg_segment_pages / _page)
        host_path = {"pipelined_patches_per_s": round(tiles_per_page * len(hp_pages) / t_pipe, 1),
                     "page_by_page_patches_per_s": round(tiles_per_page * len(hp_pages) / t_serial, 1), "pages": len(hp_pages)}

    # ---- the other arithmetic mode + live label agreement of both modes with the fp32 oracle ------
    modes, label_match, cpu_baseline, cpu_port = None, None, None, None
    if args.full and rank == 0 and world == 1:
        xy = _capi.tile_grid(PAGE_H, PAGE_W, MODEL_HW, MODEL_HW)[0]
        pick = np.linspace(0, len(xy) - 1, args.cpu_patches).astype(int)
        patches = np.stack([page0[y0:y0 + MODEL_HW, x0:x0 + MODEL_HW] for (x0, y0) in xy[pick]])
        x = (patches / 255.0).astype(np.float32)
        ref = None
        if not args.no_cpu_baseline:
            from oracle import keras_forward as kf
            kf.forward_config(cfg, weights, x[:1])                        # warm (page-in, thread pool)
            t1 = time.perf_counter()
            ref = kf.forward_config(cfg, weights, x)
            port_dt = time.perf_counter() - t1
            cpu_port = {"value": round(len(pick) / port_dt, 3), "unit": "patches/s", "cores": kf.num_threads(), "kind": "port",
                        "sample": f"{len(pick)} of the page's {len(xy)} tiles through oracle/keras_forward"}
            # torch-CPU fp32 proxy of the Keras/TF CPU path: same graph, F.conv2d / batch_norm / interpolate,
            # batch 1 (mirrors main.py:287-288: one patch per predict call) and batch 8, all host cores
            try:
                from sbb_textline_detection_amd.keras_graph import parse_model_config
                from tools.synth_model import forward_torch
                g = parse_model_config(cfg)
                import torch.nn.functional as F
                ncpu = os.cpu_count() or 1
                # torch's intra-op pool at one thread per LOGICAL cpu was measured 10x slower than the OpenMP port on the 2-socket
                # box (0.017 patches/s at 256 threads): probe one decoder-sized conv per candidate count and keep the fastest
                xa, wa = torch.randn(1, 512, 112, 112), torch.randn(128, 512, 3, 3)
                best, probe = None, {}
                with torch.no_grad():
                    for nt_ in sorted({t for t in (16, 32, 64, ncpu // 2, ncpu) if 1 <= t <= ncpu}):
                        torch.set_num_threads(nt_)
                        F.conv2d(xa, wa, padding=1)
                        t1 = time.perf_counter()
                        F.conv2d(xa, wa, padding=1)
                        probe[nt_] = time.perf_counter() - t1
                        if best is None or probe[nt_] < probe[best]:
                            best = nt_
                    nthreads = best
                    torch.set_num_threads(nthreads)
                    t1 = time.perf_counter()
                    forward_torch(g, weights, x[:1], torch.float32)      # warm (also the batch-1 estimate if the box is slow)
                    warm = time.perf_counter() - t1
                    nb1 = 2 if warm < 8 else 1
                    t1 = time.perf_counter()
                    for k in range(nb1):
                        forward_torch(g, weights, x[k:k + 1], torch.float32)
                    b1 = nb1 / (time.perf_counter() - t1)
                    nb8 = len(x) if warm < 4 else min(len(x), 2)
                    t1 = time.perf_counter()
                    q = forward_torch(g, weights, x[:nb8], torch.float32)
                    b8 = nb8 / (time.perf_counter() - t1)
                # kind "proxy": a torch-CPU fp32 forward of the same graph stands in for the reference's Keras/TF-1.15 CPU path, which cannot
                # run here; threads = the fastest of the probed counts
                cpu_baseline = {"value": round(max(b1, b8), 3), "unit": "patches/s", "cores": nthreads, "kind": "proxy",
                                "batch1_patches_per_s": round(b1, 3), f"batch{nb8}_patches_per_s": round(b8, 3), "logical_cpus": ncpu,
                                "sample": f"torch-CPU fp32, {nb1} patches at batch 1 + {nb8} at batch {nb8}; max|dsoftmax| vs oracle port "
                                          f"{float(np.abs(q - ref[:nb8]).max()):.1e}",
                                "oracle_port": {"value": cpu_port["value"], "cores": cpu_port["cores"]}}
            except Exception as e:                                        # torch CPU ops unavailable: keep the port
                cpu_baseline = dict(cpu_port, note=f"torch-CPU proxy failed: {e}")

        # label-exact modes: a label of the TIMED output may differ from the oracle's only where the oracle's own top-2 softmax margin
        # is below this (tests/gpu_common.py EXACT_MARGIN: the fp32 oracle's reassociation noise, measured worst 7e-5)
        EXACT_MARGIN = 2e-4

        def match(m, timed_map):
            """Agreement with the fp32 oracle on the sampled tiles: (a) `label_*` -- the labels the TIMED steps wrote (page 0 of the pooled
            label buffer, read back right after the timed region) inside each sampled tile's owned region (main.py:294-364: margin crop +
            last writer wins) against the oracle's argmax (main.py:290); (b) `max_abs_softmax_diff` -- seam 2 (`predict`) on the same tiles."""
            if ref is None:
                return None
            got = m.predict(x)
            srt = np.sort(ref, axis=-1)
            margin = srt[..., -1] - srt[..., -2]
            out = {"patches": int(len(pick)), "max_abs_softmax_diff": float(f"{np.abs(ref - got).max():.3g}")}
            if timed_map is None:                                       # not the page workload: seam 2's labels only
                mism = ref.argmax(-1) != got.argmax(-1)
                out.update(source="predict", label_mismatch_frac=float(f"{mism.mean():.3g}"),
                           max_oracle_margin_among_mismatches=float(f"{(margin[mism].max() if mism.any() else 0.0):.3g}"))
                return out
            from oracle import tiling
            tiles, _, _ = tiling.tile_grid(PAGE_H, PAGE_W, MODEL_HW, MODEL_HW)
            own = tiling.owner_map(PAGE_H, PAGE_W, MODEL_HW, MODEL_HW)
            n_px = n_mism = n_outside = 0
            worst = 0.0
            for i, k in enumerate(pick):
                t = tiles[int(k)]
                ys, xs = slice(t["y0"] + t["ylo"], t["y0"] + t["yhi"]), slice(t["x0"] + t["xlo"], t["x0"] + t["xhi"])
                owned = own[ys, xs] == int(k)                             # the clamped last row / column overwrites part of its neighbour
                want = ref[i, t["ylo"]:t["yhi"], t["xlo"]:t["xhi"]].argmax(-1)
                mg = margin[i, t["ylo"]:t["yhi"], t["xlo"]:t["xhi"]]
                mism = (timed_map[ys, xs] != want) & owned
                n_px += int(owned.sum())
                n_mism += int(mism.sum())
                n_outside += int((mism & (mg > EXACT_MARGIN)).sum())
                if mism.any():
                    worst = max(worst, float(mg[mism].max()))
            out.update(source="timed_output",          # page 0's mask as the TIMED steps wrote it, owned regions of the sampled tiles
                       pixels_checked=n_px, label_mismatches=n_mism, label_mismatch_frac=float(f"{n_mism / max(1, n_px):.3g}"),
                       max_oracle_margin_among_mismatches=float(f"{worst:.3g}"),
                       exact_margin=EXACT_MARGIN, label_mismatches_outside_exact_margin=n_outside)
            return out
        label_match = match(model, timed_labels0)
        modes = {args.precision: {"patches_per_s": round(value, 2), "label_match": label_match}}
        other = {"f16": "f16x3", "f16x3": "f16"}.get(args.precision)
        if other and not args.no_second_mode and workload == "page":
            m2 = make_model(other)
            step2 = build_page(m2)[0]
            tps2 = forwards_of(step2)
            n2 = max(3, args.steps // 4)
            m2.ctx.profile_reset()
            dts2 = timed(step2, n2, 1, 1)
            exec2 = executed_flops_per_patch(m2.ctx)
            timed_labels2 = page_state[id(m2)][0].cpu().numpy()
            r2, _ = roofline_of(m2)
            modes[other] = {"patches_per_s": round(tps2 * n2 / dts2[0], 2), "label_match": match(m2, timed_labels2),
                            "achieved_tflops_end_to_end": round(tps2 * n2 / dts2[0] * exec2 / 1e12, 1),
                            "roofline": {k: r2[k] for k in ("kernel", "achieved", "frac", "frac_issued", "traffic", "avg_launch_ms", "executed_share_of_launch",
                                                            "conv3x3_stages", "conv3x3_stages_incl_stage2", "all_convs") if k in r2},
                            "steps": n2}
            m2.release()
        # carried INSIDE `roofline` (which the driver's record keeps whole): north_star's one numeric target -- the 3x3 conv stages' fraction of
        # the MFMA peak in the fast fp16 mode -- and the label check of both modes on the timed output
        summary = {}
        for k, v in modes.items():
            lm = v.get("label_match") or {}
            rr = roofline if k == args.precision else v.get("roofline", {})
            summary[k] = {"patches_per_s": v["patches_per_s"], "label_exact_mode": k == "f16x3",
                          "conv3x3_frac": rr.get("conv3x3_stages", {}).get("frac"),
                          "conv3x3_frac_incl_stage2": rr.get("conv3x3_stages_incl_stage2", {}).get("frac"),
                          "all_convs_frac": rr.get("all_convs", {}).get("frac"),
                          "label_mismatches_outside_exact_margin": lm.get("label_mismatches_outside_exact_margin"),
                          "label_mismatch_frac": lm.get("label_mismatch_frac"), "max_abs_softmax_diff": lm.get("max_abs_softmax_diff")}
        roofline["modes"] = summary

    exit_code = 0
    extras = None
    if args.full and rank == 0 and world == 1 and workload == "page" and not args.no_extras:
        extras = {}
        # one page per step (BASELINE configs[1] literally: ONE 3500x2500 page = 70 tiles per call)
        keep = args.pages_per_step
        args.pages_per_step = 1
        step1 = build_page(model)[0]
        tps1 = forwards_of(step1)
        n1 = max(10, args.steps)
        d1 = timed(step1, n1, 2, 1)[0]
        args.pages_per_step = keep
        extras["one_page_patches_per_s"] = round(tps1 * n1 / d1, 1)
        extras["one_page_ms"] = round(d1 / n1 * 1e3, 3)
        # BASELINE configs[2]: border (whole image) + layout (Otsu'd, 4 classes) + textline on ONE page, models resident
        try:
            step3, calls3, desc3 = build_pipeline3(model)[:3]
            tps3 = forwards_of(step3)
            n3 = max(5, args.steps // 2)
            d3 = timed(step3, n3, 2, 1)[0]
            extras["pipeline3_ms_per_page"] = round(d3 / n3 * 1e3, 3)
            extras["pipeline3_forwards_per_page"] = tps3
            extras["pipeline3_reference_calls_per_page"] = calls3
            extras["pipeline3_patches_per_s"] = round(tps3 * n3 / d3, 1)
            extras["pipeline3_host_contour_fallbacks_per_page"] = round(fallbacks_of_pipeline3() / float(n3 + 2), 2)
            parts = {}
            for name, fn in step3.stages.items():                      # each piece alone: where the page's milliseconds go
                fn(); torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(n3):
                    fn()
                torch.cuda.synchronize()
                parts[name] = round((time.perf_counter() - t0) / n3 * 1e3, 3)
            extras["pipeline3_breakdown"] = parts
        except Exception as e:                                         # never lose the headline over a side measurement
            extras["pipeline3_error"] = repr(e)

    if rank == 0:
        out = {
            "metric": "segmented patches/sec (448x448x3) per GPU + per-pixel label-map match vs ref",
            "value": round(value, 2), "unit": "patches/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(dt / args.steps * 1e3, 3), "higher_is_better": True, "scaling": scaling,
            "vs_baseline": None, "dtype": args.precision, "data": "synthetic",
            "config": {"workload": workload_desc, "workload_id": workload,
                       "tiles_per_step": tiles_per_step, "forwards_per_step": tiles_per_step,
                       "reference_calls_per_step": reference_calls_per_step, "dedupe": tiles_per_step != reference_calls_per_step,
                       "max_batch": args.max_batch,
                       "lanes": int(os.environ.get("SBBSEG_LANES", "2")),
                       "owned_regions": int(os.environ.get("SBBSEG_OWNED_REGIONS", "1")),
                       "exchange": ("RCCL all_gather of u8 label maps" if backend == "nccl" else f"host-staged all_gather ({backend})") if world > 1 else "none",
                       # reference formulation (whole tiles, 3x3 convs over the upsampled + concatenated input) vs what the handle executed:
                       # owned-region launches skip the decoder pixels the page stitch would discard (main.py:294-364)
                       "flops_per_patch": 2 * model.plan.macs_per_patch(),
                       "executed_flops_per_patch": round(exec_flops),
                       "executed_share": round(exec_flops / (2 * model.plan.macs_per_patch()), 4)},
            "repeats": {"patches_per_s": [round(r, 2) for r in rates], "timed_region_s": [round(t, 3) for t in dts]},
            "patches_per_s_per_gpu": round(value / world, 2),
            "achieved_tflops_end_to_end": round(value / world * exec_flops / 1e12, 1),
            "reference_formulation_tflops_end_to_end": round(value / world * 2 * model.plan.macs_per_patch() / 1e12, 1),
            "roofline": roofline, "cpu_baseline": cpu_baseline, "label_match": label_match,
            "modes": {k: {kk: vv for kk, vv in v.items() if not (k == args.precision and kk == "label_match")} for k, v in modes.items()} if modes else None,
            "exchange": exchange,
            "per_rank": per_rank, "ranks_seen": ranks_seen, "host_path": host_path, "extras": extras, "batch64": batch64,
        }
        if world > 1:
            out["config"]["collective"] = "capi (sbbseg_allgather_labels_dev)" if collective == "capi" else "torch.distributed (%s)" % backend
        # a label-exact mode whose TIMED output differs from the oracle outside the oracle's own near-ties fails the run
        for mode_name, mm in (modes or {}).items():
            lm = mm.get("label_match") or {}
            if mode_name == "f16x3" and lm.get("label_mismatches_outside_exact_margin", 0) > 0:
                out["label_check_failed"] = True
                exit_code = 3
        line = json.dumps(out, separators=(",", ":"))
        if len(line) > 6000 and world == 1:
            # the driver's record keeps a bounded tail of the line: shed the side measurements first, never the contract's keys
            for key in ("host_path", "batch64", "extras", "label_match"):
                if len(line) <= 6000:
                    break
                side = out.pop(key, None)
                if side is not None and os.environ.get("SBBSEG_BENCH_SIDE"):
                    with open(os.environ["SBBSEG_BENCH_SIDE"], "a") as f:
                        f.write(json.dumps({key: side}) + "\n")
                line = json.dumps(out, separators=(",", ":"))
        print(line)
        if os.environ.get("SBBSEG_BENCH_OPS") and args.full:
            with open(os.environ["SBBSEG_BENCH_OPS"], "w") as f:
                json.dump(per_op, f, indent=1)
    if world > 1:
        if comm_state["ctx"] is not None:
            comm_state["ctx"].comm_destroy()
        dist.barrier()
        dist.destroy_process_group()
    model.release()
    if exit_code:
        raise SystemExit(exit_code)


if __name__ == "__main__":
    main()
