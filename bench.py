#!/usr/bin/env python3
"""Headline benchmark: frames/sec of the Phase-2 DETR detect path (BASELINE.json: detr-resnet-50, batch 8, 800x1333).

    python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR]

N > 1 works both ways: started by ``torch.distributed.run`` (RANK / LOCAL_RANK / WORLD_SIZE in the environment: one rank per
GPU) or as a plain ``python bench.py --gpus N`` — then this process, before it imports torch or touches a GPU, starts N fresh
child processes of itself with that environment, waits for them, and exits non-zero if any of them failed (rank 0 prints the
JSON line on the shared stdout).

A step = one pass of the hot path over one batch of synthetic frames per rank: uint8 BGR frames already resident in HBM ->
preprocess -> ResNet-50 -> encoder/decoder -> heads -> device post-process -> detection records; with N > 1 every rank detects
its own shard of the global batch (8 frames per rank, weak scaling) and the records are all-gathered over RCCL/xGMI to every
rank inside the step; rank 0 (the orchestrator) then runs the person filter + NMS (`opd_person_nms_batch`) on the gathered
records, so a step ends with what `DetectionPhase` consumes.  Rank 0 prints ONE JSON line.

Steps are submitted asynchronously to `--streams` detector handles per GPU (default 3: own stream / workspace / graph, one
shared copy of the weights), so up to three batches of 8 are in flight per GPU; every step's records reach host memory inside
the timed region, which is bracketed by barrier + device synchronisation.  The line also carries a `serial` record — a short
leg with ONE handle (a single-stream caller's kernel plan) and one blocking call per step — and both profiling legs run on
that handle: `stage_ms` / `roofline.graph_ms_per_step` from stage marks recorded INSIDE the replayed graph
(`roofline_serial.closes`: graph_ms_per_step <= serial.ms_per_step), `roofline` from HIP event pairs around every launch of
an eagerly launched forward (true kernel durations; their sum, `kernel_ms_per_step`, carries ~10 us of eager dispatch and
event overhead per launch and therefore exceeds the step it dissects).

``--dump-outputs DIR`` writes what the timed path handed its caller in its last timed step (rank 0's records after the person
filter + NMS, see `dump_outputs`) as ``DIR/<name>.npy``.  Frames and weights are seeded, so two builds run with the same arguments
can be compared output for output.
"""

from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

PEAK_MFMA_TFLOPS = 2500.0  # dense fp16/bf16 MFMA, /opt/skills/guides/MI355X_MICROARCH.md §Chip-level parameters
PEAK_HBM_GBS = 8000.0


def launch_ranks(n: int, argv, env=None, script=None) -> int:
    """Parent side of ``python bench.py --gpus N``: N child processes (one rank per GPU) with the torch.distributed
    environment; returns 0 only if every rank exited 0.  Runs before torch is imported: nothing here touches a GPU, and no
    process that has initialised a GPU is ever exec'ed or re-exec'ed.  Rank 0 inherits stdout (its JSON line is the output);
    the other ranks' stdout goes to stderr."""
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    procs = []

    def on_signal(signum, _frame):   # the parent is being stopped: take the ranks it started down with it (never orphan GPU children)
        for pr in procs:
            if pr.poll() is None:
                pr.terminate()
        sys.exit(128 + signum)

    import signal
    for sig in (signal.SIGTERM, signal.SIGINT):
        signal.signal(sig, on_signal)
    for r in range(n):
        e = dict(os.environ if env is None else env)
        e.update({"RANK": str(r), "LOCAL_RANK": str(r), "WORLD_SIZE": str(n), "LOCAL_WORLD_SIZE": str(n),
                  "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port)})
        e.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")   # dmabuf IPC: RCCL needs it on this driver
        procs.append(subprocess.Popen([sys.executable, script or os.path.abspath(__file__)] + list(argv), env=e,
                                      stdout=None if r == 0 else sys.stderr))
    rc = 0
    live = set(range(n))
    while live:
        for r in sorted(live):
            code = procs[r].poll()
            if code is None:
                continue
            live.discard(r)
            if code != 0 and rc == 0:
                rc = code if code > 0 else 1
                print(f"bench.py: rank {r} exited with {code}; stopping the other ranks", file=sys.stderr, flush=True)
                for o in live:   # exactly the processes started above
                    procs[o].terminate()
        time.sleep(0.05)
    return rc


def cpu_baseline(path: str, H: int, W: int, batch: int = 4, iters: int = 3) -> dict:
    """The oracle (CPU fp32 restatement, torch CPU backend) on a bounded sample of the same workload (BASELINE configs[0])."""
    import torch

    from office_person_detection_vit_amd.frames import structured_frame
    from office_person_detection_vit_amd.weights import load_safetensors
    from oracle import detr_oracle as O

    # use the host cores this process may actually run on (the GPU box shares its CPUs between boxes)
    try:
        ncpu = len(os.sched_getaffinity(0))
    except AttributeError:
        ncpu = os.cpu_count() or 1
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            ncpu = max(1, min(ncpu, int(int(quota) / int(period))))
    except Exception:
        pass
    torch.set_num_threads(ncpu)
    w = O.to_torch(load_safetensors(path))
    frames = [structured_frame(H, W, 1234 + i) for i in range(batch)]
    times = []
    for it in range(iters + 1):  # first iteration is the warm-up
        t0 = time.perf_counter()
        pv, pm = O.preprocess(frames)
        lg, bx, _ = O.forward(w, pv, pm)
        res = O.post_process_object_detection(lg.numpy(), bx.numpy(), 0.5, [(H, W)] * batch)
        for r in res:
            O.person_detections(r, 0.4)
        times.append(time.perf_counter() - t0)
    best = min(times[1:])
    return {"value": round(batch / best, 4), "unit": "frames/s", "cores": int(torch.get_num_threads()), "kind": "port",
            "sample": f"oracle/detr_oracle.py (torch CPU fp32), detr-resnet-50, {batch}x{H}x{W} frames, forward + post-process + "
                      f"person filter/NMS, 1 warm-up + {iters} timed iterations, best iteration {best:.2f} s "
                      f"(all: {', '.join(f'{t:.2f}' for t in times[1:])})"}


def dump_outputs(out_dir: str, recs, counts, Q: int) -> dict:
    """The detections of one step as a caller of the path receives them: frame f owns records [f * Q, f * Q + counts[f]) of `recs`
    (opd_det viewed as int32 [n][8]; a negative count marks a padding slot).  Every field goes to its own float32 / float64 file
    (integer fields as float64, exact), records of all frames concatenated in frame order; at most a few hundred KB."""
    import numpy as np

    counts = np.asarray(counts, dtype=np.int64).reshape(-1)
    recs = np.asarray(recs, dtype=np.int32).reshape(-1, 8)
    rows = [recs[f * Q:f * Q + max(int(c), 0)] for f, c in enumerate(counts)]
    r = np.ascontiguousarray(np.concatenate(rows) if rows else np.zeros((0, 8), np.int32))
    fl = r.view(np.float32)
    arrays = {"boxes_xyxy": np.ascontiguousarray(fl[:, 0:4]),   # pixels of the original frame
              "scores": np.ascontiguousarray(fl[:, 4]),
              "labels": r[:, 5].astype(np.float64),
              "query_index": r[:, 6].astype(np.float64),
              "frame": r[:, 7].astype(np.float64),
              "counts": counts.astype(np.float64)}   # per frame slot of the global batch
    os.makedirs(out_dir, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), a)
    return {"dir": out_dir, "arrays": {k: list(a.shape) for k, a in arrays.items()}}


def _capi_unique_id(lib):
    buf = C.create_string_buffer(128)
    if lib.opd_comm_unique_id(buf) != 0:
        raise RuntimeError(lib.opd_last_error().decode())
    return buf.raw


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=1000)  # 2.8 s timed (windows of 20 / 1000 / 3000 steps read within 2 % of each other; a
                                                        # 200-step window read ~4 % low on the boxes of round 3, cause not established)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=8, help="frames per GPU per step")
    ap.add_argument("--height", type=int, default=800)
    ap.add_argument("--width", type=int, default=1333)
    ap.add_argument("--arch", choices=["r50", "r101"], default="r50", help="backbone depth (r101 = BASELINE configs[3]; not the headline workload)")
    ap.add_argument("--dtype", choices=["f16", "bf16"], default="f16",
                    help="16-bit operand type of the device path: f16 (default: fp16 operands, fp32 accumulate; meets the 1e-3 box tolerance) or "
                         "bf16 (OPD_FLAG_BF16: the type BASELINE configs[1] names; same MFMA rate, looser parity: DESIGN.md section 3)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--streams", type=int, default=int(os.environ.get("OPD_BENCH_STREAMS", "3")),
                    help="detector handles (own stream, workspace and graph each) that take the steps in turn: the low-"
                         "occupancy tail of step i (decoder, heads) overlaps the trunk of step i+1")
    ap.add_argument("--sync-steps", action="store_true",
                    help="one blocking detect call per step (default: steps are submitted asynchronously, results of step i-1 are "
                         "fetched while step i computes)")
    ap.add_argument("--serial-steps", type=int, default=30, help="steps of the serial cross-check leg (0 = skip)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step returned to its caller (rank 0's detection records "
                         "after NMS) as DIR/<name>.npy (float32 / float64)")
    ap.add_argument("--cpu-rehearsal", action="store_true",
                    help="no GPU: exercise launch, rendezvous (gloo), the step loop's collective and the rank-0 JSON with the "
                         "device compute left out — a plumbing test, never a measurement")
    args = ap.parse_args(argv)
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    return args


def main() -> int:
    args = parse_args()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        return launch_ranks(args.gpus, sys.argv[1:])
    # (ranks started by torch.distributed.run inherit their launcher's environment; this driver supports dmabuf IPC only, and RCCL / device-memory
    #  sharing across processes fails without the switch -- set before anything loads the HIP runtime)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

    # stdout carries the ONE JSON line and nothing else: libraries that print to fd 1 (gloo's connection banner, a chatty
    # runtime) are redirected to stderr for the rest of the process
    sys.stdout.flush()
    json_out = os.fdopen(os.dup(1), "w")
    os.dup2(2, 1)

    import numpy as np
    import torch
    import torch.distributed as dist

    from office_person_detection_vit_amd import _capi
    from office_person_detection_vit_amd.frames import structured_frame
    from office_person_detection_vit_amd.weights import DetrArch, ensure_weight_file

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    rehearsal = args.cpu_rehearsal
    if not rehearsal and not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: no HIP device visible (there is no CPU fallback)")
    # OPD_BENCH_BACKEND=gloo is a REHEARSAL mode for a one-GPU box: every rank uses device 0 and the records travel through
    # host memory; it exercises the multi-rank control flow (barriers, max-over-ranks timing, rank-0 JSON), not RCCL.
    backend = "gloo" if rehearsal else os.environ.get("OPD_BENCH_BACKEND", "nccl")
    device_index = local_rank if backend == "nccl" else 0
    if not rehearsal:
        torch.cuda.set_device(device_index)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", device_index))
        else:
            dist.init_process_group(backend)

    B, H, W = args.batch, args.height, args.width
    lib = _capi.load_library()
    Q = 100
    handles = []
    path = None
    if not rehearsal:
        cache = os.environ.get("OPD_WEIGHT_CACHE", "/tmp/opd_weights")
        arch = DetrArch.resnet101() if args.arch == "r101" else DetrArch.resnet50()
        if rank == 0:
            path = ensure_weight_file(cache, arch, 0, 1.0, args.arch)
        if world > 1:
            dist.barrier()
        path = ensure_weight_file(cache, arch, 0, 1.0, args.arch)
        # several handles keep batches in flight: the library may choose kernels for throughput (include/opd_detr.h, OPD_FLAG_MULTI_STREAM)
        cfg = _capi.OpdConfig(struct_size=C.sizeof(_capi.OpdConfig), max_batch=B, max_height=H, max_width=W,
                              flags=(_capi.OPD_FLAG_MULTI_STREAM if args.streams > 1 else 0) | (_capi.OPD_FLAG_BF16 if args.dtype == "bf16" else 0))
        handle = C.c_void_p()
        _capi.check(lib.opd_detr_create(C.byref(cfg), path.encode(), device_index, C.byref(handle)), "opd_detr_create")
        info = _capi.OpdModelInfo()
        _capi.check(lib.opd_detr_info(handle, C.byref(info)), "opd_detr_info")
        handles = [handle]
        for _ in range(1, max(1, args.streams)):
            hx = C.c_void_p()   # same weights in HBM, own stream / workspace / graph
            _capi.check(lib.opd_detr_clone(handle, C.byref(hx)), "opd_detr_clone")
            handles.append(hx)
        Q = info.num_queries
    NS = max(1, len(handles))
    dev = "cpu" if rehearsal else "cuda"
    # N > 1: the path's exchange step runs inside the C-ABI (opd_comm_*: ncclAllGather on each handle's own stream, one host wait per
    # step); torch.distributed carries the 128-byte unique ids at set-up, the barriers and the max-over-ranks of the timing.  The
    # torch.distributed all-gather of rounds 1-3 remains for the gloo rehearsal (ranks sharing one device cannot form an RCCL
    # communicator) and as the fallback should communicator creation fail on a node.
    # ONE communicator per rank (default): handle 0 creates it, the other handles attach LANES to it (opd_comm_attach); every all-gather of
    # the rank is enqueued on the communicator's own stream in submission order, the same order on every rank (step i uses lane i mod NS).
    # OPD_BENCH_COMMS=per-handle: one communicator per handle (round 4's arrangement: collectives of different communicators on unordered
    # streams; kept as a switch for a node where it can be compared, never the default).
    # Set-up protocol: (1) every rank checks that librccl can be resolved and the ranks AGREE on it (all_reduce) before anyone enters a
    # collective initialisation -- a rank that cannot take part must not leave its peers blocked in ncclCommInitRank; (2) rank 0's unique
    # id(s) travel through the process group; (3) ncclCommInitRank under a watchdog: failure or a stall past OPD_BENCH_COMM_TIMEOUT seconds
    # ends this rank with a non-zero exit code (the parent stops the others) -- there is no fallback from a half-initialised communicator.
    comms, exchange = [], "none"
    force_comm = os.environ.get("OPD_BENCH_FORCE_COMM") == "1"   # test switch: the native exchange over a ONE-rank communicator
    if world > 1:
        exchange = "torch.distributed"
    if not rehearsal and ((world > 1 and backend == "nccl") or (world == 1 and force_comm)) and os.environ.get("OPD_BENCH_EXCHANGE", "native") == "native":
        avail = 1 if lib.opd_comm_available() == 0 else 0
        if not avail:
            print(f"bench.py: rank {rank}: {lib.opd_last_error().decode()}", file=sys.stderr, flush=True)
        if world > 1:
            t_av = torch.tensor([avail], device="cuda")
            dist.all_reduce(t_av, op=dist.ReduceOp.MIN)   # every rank or none, decided before any collective set-up
            avail = int(t_av.item())
        if avail:
            per_handle = os.environ.get("OPD_BENCH_COMMS", "shared") == "per-handle"
            ids = [[bytes(_capi_unique_id(lib)) for _ in range(NS if per_handle else 1)] if rank == 0 else None]
            if world > 1:
                dist.broadcast_object_list(ids, src=0)
            import threading
            limit = float(os.environ.get("OPD_BENCH_COMM_TIMEOUT", "120"))

            def stalled():
                print(f"bench.py: rank {rank}: communicator set-up did not finish within {limit:.0f} s; giving up", file=sys.stderr, flush=True)
                os._exit(3)

            dog = threading.Timer(limit, stalled)
            dog.daemon = True
            dog.start()
            try:
                for k, hx in enumerate(handles):
                    cx = C.c_void_p()
                    if per_handle or k == 0:
                        _capi.check(lib.opd_comm_create(ids[0][k if per_handle else 0], rank, world, hx, C.byref(cx)), "opd_comm_create")
                    else:
                        _capi.check(lib.opd_comm_attach(comms[0], hx, C.byref(cx)), "opd_comm_attach")
                    comms.append(cx)
            except Exception as e:   # noqa: BLE001 -- inside a collective initialisation there is nothing to fall back to
                print(f"bench.py: rank {rank}: communicator set-up failed: {e}", file=sys.stderr, flush=True)
                os._exit(3)
            finally:
                dog.cancel()
            exchange = ("native (opd_comm_*: one communicator per handle)" if per_handle else
                        f"native (opd_comm_*: ONE communicator per rank, {NS} lane(s), all-gathers on its own stream in submission order)")
        else:
            print("bench.py: librccl not available on every rank; the exchange runs on torch.distributed", file=sys.stderr, flush=True)

    # synthetic office-camera frames, resident in HBM before the timed region (torch = device memory plumbing only)
    d_frames = None
    if not rehearsal:
        frames = np.stack([structured_frame(H, W, 1234 + rank * B + i) for i in range(B)])
        d_frames = torch.from_numpy(frames).cuda()
    # one flat int32 buffer per rank: B*Q records (opd_det = 8 x 4 bytes) followed by the B per-frame counts, so that the
    # path's exchange step is ONE all-gather
    NREC = B * Q * 8
    d_flats = [torch.zeros((NREC + B,), dtype=torch.int32, device=dev) for _ in range(2 * NS)]   # rotating output buffers
    gdev = "cuda" if backend == "nccl" else "cpu"
    g_flat = torch.zeros((world * (NREC + B),), dtype=torch.int32, device=gdev) if world > 1 else None
    hw = np.asarray([[H, W]] * B, dtype=np.int32)
    DetP, I32P = C.POINTER(_capi.OpdDet), C.POINTER(C.c_int32)
    if not rehearsal:
        torch.cuda.synchronize()   # the buffers above were filled on torch's stream; the library writes them from its own streams

    g_recs = np.zeros((world * B * Q, 8), np.int32)
    g_counts = np.zeros((world * B,), np.int32)
    last = {}   # rank 0: the records + counts of the most recently collected step (what --dump-outputs writes)

    def collect(buf, j=0):
        """records (+ counts) of one finished step -> the orchestrator's host memory (the path's one exchange step for N > 1),
        then the host tail of the path on rank 0: person filter + greedy NMS on every gathered frame, in place"""
        if comms:   # native exchange: the all-gather was enqueued with the step; this is the step's one host wait
            _capi.check(lib.opd_comm_wait(comms[j % NS], g_recs.ctypes.data_as(DetP), g_counts.ctypes.data_as(I32P)), "opd_comm_wait")
            if rank != 0:
                return None
            recs, counts = g_recs, g_counts
        elif world > 1:
            dist.all_gather_into_tensor(g_flat, buf if backend == "nccl" else buf.cpu())
            if rank != 0:
                # `buf` is a rotating buffer that a later step's post-process kernel rewrites from the LIBRARY's stream, which knows
                # nothing of torch's / RCCL's streams: host-wait here until the collective has read it (rank 0 waits in .cpu() below)
                if backend == "nccl":
                    torch.cuda.current_stream().synchronize()
                return None
            g = g_flat.cpu().view(world, NREC + B).numpy()
            recs = np.ascontiguousarray(g[:, :NREC]).reshape(world * B * Q, 8)
            counts = np.ascontiguousarray(g[:, NREC:]).reshape(world * B)
        else:
            h = buf.cpu().numpy()
            recs, counts = h[:NREC].reshape(B * Q, 8), h[NREC:]
        _capi.check(lib.opd_person_nms_batch(recs.ctypes.data_as(DetP), counts.ctypes.data_as(I32P), len(counts), Q, 1, 0.4),
                    "opd_person_nms_batch")
        last["recs"], last["counts"] = recs, counts
        return counts

    def detect_blocking(h, buf):
        rc = lib.opd_detr_detect(h, C.c_void_p(d_frames.data_ptr()), _capi.OPD_PIXELS_U8_BGR_HWC, _capi.OPD_MEM_DEVICE,
                                 B, H, W, 0.5, hw.ctypes.data_as(C.c_void_p), C.cast(C.c_void_p(buf.data_ptr()), DetP),
                                 C.cast(C.c_void_p(buf[NREC:].data_ptr()), I32P))
        _capi.check(rc, "opd_detr_detect")

    def submit(i):
        """enqueue step i on a handle's stream (forward + post-process into a rotating buffer) and return its ticket"""
        if rehearsal:
            return 0
        if comms:   # forward -> post-process into the communicator's send buffer -> ncclAllGather -> copy to pinned memory: all enqueued
            cx = comms[i % NS]
            _capi.check(lib.opd_comm_begin(cx, B), "opd_comm_begin")
            _capi.check(lib.opd_comm_detect(cx, 0, C.c_void_p(d_frames.data_ptr()), _capi.OPD_PIXELS_U8_BGR_HWC, _capi.OPD_MEM_DEVICE, B, H, W, 0.5,
                                            hw.ctypes.data_as(C.c_void_p)), "opd_comm_detect")
            _capi.check(lib.opd_comm_exchange(cx), "opd_comm_exchange")
            return -1
        buf = d_flats[i % (2 * NS)]
        ticket = C.c_int()
        rc = lib.opd_detr_detect_async(handles[i % NS], C.c_void_p(d_frames.data_ptr()), _capi.OPD_PIXELS_U8_BGR_HWC, _capi.OPD_MEM_DEVICE,
                                       B, H, W, 0.5, hw.ctypes.data_as(C.c_void_p), C.cast(C.c_void_p(buf.data_ptr()), DetP),
                                       C.cast(C.c_void_p(buf[NREC:].data_ptr()), I32P), C.byref(ticket))
        _capi.check(rc, "opd_detr_detect_async")
        return ticket.value

    def run_steps(n, blocking=False):
        """n steps; every step's records reach host memory.  Pipelined form: step i is submitted before step i-NS is collected."""
        out = None
        if blocking and not rehearsal:
            for _ in range(n):
                if comms:
                    submit(0)
                else:
                    detect_blocking(handles[0], d_flats[0])
                out = collect(d_flats[0], 0)
            return out
        # NS steps stay submitted ahead (one per handle); step i - NS is collected right after step i has been submitted.  Plain handles
        # rotate 2 NS output buffers; a communicator lane owns TWO send / receive buffer sets (csrc/opd_comm.cpp: LaneSet), so step i fills
        # one while step i - NS travels in the other -- the same loop either way.  (Round 4's lanes had one set, and this loop raised
        # OPD_ESTATE at step NS: ADVICE r4.)
        tickets = {}
        for i in range(n + NS):
            if i < n:
                tickets[i] = submit(i)
            j = i - NS
            if j >= 0:
                t = tickets.pop(j)
                if not rehearsal and not comms:
                    _capi.check(lib.opd_detr_wait(handles[j % NS], t), "opd_detr_wait")
                out = collect(d_flats[j % (2 * NS)], j)
        return out

    def sync():
        if not rehearsal:
            torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
            if not rehearsal:
                torch.cuda.synchronize()

    if args.warmup:
        run_steps(args.warmup, args.sync_steps)
    sync()
    t0 = time.perf_counter()
    counts = run_steps(args.steps, args.sync_steps)
    sync()
    elapsed = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([elapsed], dtype=torch.float64, device=gdev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    # the last timed step's outputs, written before any later leg reuses the buffers they live in
    dumped = dump_outputs(args.dump_outputs, last["recs"], last["counts"], Q) if args.dump_outputs and rank == 0 else None

    # ---- sustained leg: the same handles over a window of >= 2 s.  The driver's --steps 20 times 55 ms of GPU work; this leg, in the same
    # JSON line, shows whether that burst is representative (all ranks take part: it is bracketed like the timed region).
    sustained = None
    if not rehearsal and args.steps < 750 and os.environ.get("OPD_BENCH_SUSTAINED", "1") != "0":
        n_sus = max(750, int(2.2 / max(elapsed / args.steps, 1e-6)))
        sync()
        ts0 = time.perf_counter()
        run_steps(n_sus, args.sync_steps)
        sync()
        e_sus = time.perf_counter() - ts0
        if world > 1:
            t = torch.tensor([e_sus], dtype=torch.float64, device=gdev)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            e_sus = float(t.item())
        f_sus = B * world * n_sus / e_sus
        ratio = f_sus / (B * world * args.steps / elapsed)
        sustained = {"steps": n_sus, "seconds": round(e_sus, 3), "ms_per_step": round(1e3 * e_sus / n_sus, 3), "frames_per_s": round(f_sus, 2),
                     "ratio_to_value": round(ratio, 4), "agrees_within_3pct": bool(abs(ratio - 1.0) <= 0.03)}

    # ---- rank-local legs (no collective from here to the final barrier: the other ranks wait there) ---------------------
    roof = serial = stage_ms = None
    if rank == 0 and not rehearsal:
        handle = handles[0]
        # serial cross-check: ONE handle, one blocking call per step (forward + post-process + records to host + NMS).  It is a handle of
        # its own, configured the way a single-stream caller would (no OPD_FLAG_MULTI_STREAM), not one of the handles of the timed leg.
        if args.serial_steps > 0:
            shandle = handle
            if args.streams > 1:
                scfg = _capi.OpdConfig(struct_size=C.sizeof(_capi.OpdConfig), max_batch=B, max_height=H, max_width=W,
                                       flags=_capi.OPD_FLAG_BF16 if args.dtype == "bf16" else 0)
                shandle = C.c_void_p()
                _capi.check(lib.opd_detr_create(C.byref(scfg), path.encode(), device_index, C.byref(shandle)), "opd_detr_create")
                handles.append(shandle)   # (destroyed with the others)
            detect_blocking(shandle, d_flats[0])
            torch.cuda.synchronize()
            ts = time.perf_counter()
            for _ in range(args.serial_steps):
                detect_blocking(shandle, d_flats[0])
                h = d_flats[0].cpu().numpy()
                recs, cnts = h[:NREC].reshape(B * Q, 8), h[NREC:]
                lib.opd_person_nms_batch(recs.ctypes.data_as(DetP), cnts.ctypes.data_as(I32P), B, Q, 1, 0.4)
            torch.cuda.synchronize()
            s_ms = 1e3 * (time.perf_counter() - ts) / args.serial_steps
            serial = {"streams": 1, "steps": args.serial_steps, "ms_per_step": round(s_ms, 3), "frames_per_s": round(B / s_ms * 1e3, 1)}
        # Both profiling legs run on the handle of the serial leg (a single-stream caller's kernel plan), so that they describe the
        # mode that leg timed:  (a) stage marks INSIDE the replayed graph (opd_detr_set_profiling 2): the device time of a step as a
        # caller gets it — their sum must not exceed serial.ms_per_step;  (b) HIP event pairs around every launch (mode 1: eager
        # launches; the events and the eager dispatch add ~10 us per launch, so this sum exceeds the step it dissects).
        phandle = handles[-1] if args.serial_steps > 0 else handle
        stage_graph = None
        _capi.check(lib.opd_detr_set_profiling(phandle, 2), "opd_detr_set_profiling")
        sg = np.zeros(8)
        NREP = 20
        for it in range(2 + NREP):   # eager, capture, then NREP replays (the serial leg's own 30-step window: averaged over as many steps)
            detect_blocking(phandle, d_flats[0])
            if it >= 2:
                s8 = (C.c_float * 8)()
                _capi.check(lib.opd_detr_stage_times(phandle, s8), "opd_detr_stage_times")
                sg += np.asarray(list(s8))
        if sg.sum() > 0:
            stage_graph = [round(float(v), 4) for v in sg / NREP]
        # roofline of the dominant kernel: HIP event pairs around every launch on the library's stream (eager, serial)
        handle = phandle
        _capi.check(lib.opd_detr_set_profiling(handle, 1), "opd_detr_set_profiling")
        ms_acc, st_acc = np.zeros(4), np.zeros(8)
        fl, ln = np.zeros(4), np.zeros(4, dtype=np.int64)
        reps = 3
        for _ in range(reps):
            detect_blocking(handle, d_flats[0])
            ms4, l4, f4, s8 = (C.c_float * 4)(), (C.c_int32 * 4)(), (C.c_double * 4)(), (C.c_float * 8)()
            _capi.check(lib.opd_detr_kernel_times(handle, ms4, l4, f4), "opd_detr_kernel_times")
            _capi.check(lib.opd_detr_stage_times(handle, s8), "opd_detr_stage_times")
            ms_acc += np.asarray(list(ms4)); fl = np.asarray(list(f4)); ln = np.asarray(list(l4)); st_acc += np.asarray(list(s8))
        ms_avg = ms_acc / reps
        # the same event pairs by kernel instantiation (opd_detr_kernel_table; the last of the `reps` forwards): the single largest kernel
        ktab = (_capi.OpdKernelStat * 64)()
        kcount = C.c_int(0)
        _capi.check(lib.opd_detr_kernel_table(handle, ktab, 64, C.byref(kcount)), "opd_detr_kernel_table")
        krows = [{"kernel": ktab[i].name.decode(), "launches": int(ktab[i].launches), "ms": float(ktab[i].ms), "flops": float(ktab[i].flops)}
                 for i in range(min(kcount.value, 64))]
        stage_eager = [round(float(v), 4) for v in st_acc / reps]
        stage_ms = stage_graph if stage_graph is not None else stage_eager
        _capi.check(lib.opd_detr_set_profiling(handle, 0), "opd_detr_set_profiling")
        # dominant kernel = the implicit-GEMM family (backbone convolutions incl. the fused tails + transformer linears): classes 0 and 1
        k_ms = float(ms_avg[0] + ms_avg[1])
        k_fl = float(fl[0] + fl[1])
        k_n = int(ln[0] + ln[1])
        achieved = k_fl / (k_ms * 1e-3) / 1e12 if k_ms > 0 else 0.0
        # HBM bytes per launch of the same kernel family from the committed rocprofv3 PMC passes (FETCH_SIZE / WRITE_SIZE
        # in separate runs, gfx950 x2 fetch correction: tools/pmc_traffic.py) — valid for the default 8 x 800x1333 workload
        traffic = None
        for name in ("r05_pmc_traffic.json", "r04_pmc_traffic.json", "r03_pmc_traffic.json", "r02_pmc_traffic.json", "r01_pmc_traffic.json"):
            tpath = os.path.join(ROOT, "profiles", name)
            if os.path.exists(tpath) and (B, H, W) == (8, 800, 1333) and args.arch == "r50":
                traffic = round(json.load(open(tpath))["conv_gemm_family"]["bytes_per_launch"])
                break
        roof = {"bound": "mfma", "kernel": "implicit-GEMM family (conv_gemm_dma_kernel, btail_kernel, btail256_kernel, gemm_ln256_ring/os_kernel, enc_ffn_kernel, gemm_k256_kernel, stem_pool2_kernel)",
                "achieved": round(achieved, 2), "peak": PEAK_MFMA_TFLOPS,
                "unit": "TFLOP/s", "frac": round(achieved / PEAK_MFMA_TFLOPS, 4), "traffic": traffic,
                "launches_per_step": k_n, "avg_launch_us": round(1e3 * k_ms / max(k_n, 1), 2),
                "flops_per_launch": round(k_fl / max(k_n, 1)),
                "family_ms_per_step": round(k_ms, 4),
                "kernel_ms_per_step": round(float(ms_avg.sum()), 4),   # every launch of a serial forward + post-process, EAGER mode (event pair per launch)
                "graph_ms_per_step": round(float(sum(stage_graph)), 4) if stage_graph else None,   # the same forward inside the replayed graph (stage marks in the graph)
                "stage_ms_eager": stage_eager,
                "by_class_ms": {"conv": round(float(ms_avg[0]), 4), "linear": round(float(ms_avg[1]), 4),
                                "attention": round(float(ms_avg[2]), 4), "other": round(float(ms_avg[3]), 4)},
                "traffic_source": "committed profile (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of this workload: profiles/*_pmc_traffic.json), not measured in this run",
                "peak_note": "peak = 2500 TFLOP/s is 1024 FLOP/clk/SIMD at 2.4 GHz; back-to-back MFMAs from registers on random fp16 operands hold "
                             "1.90-1.91 PFLOP/s at 1.91-1.97 GHz on this part (tools/microbench/mfma_peak.hip, profiles/r05_microbench_mfma_peak.txt): "
                             "no k-loop can read above 0.76 of `peak`"}
        gemm_rows = [r for r in krows if r["flops"] > 0 and r["ms"] > 0]
        if gemm_rows:
            d = max(gemm_rows, key=lambda r: r["ms"])
            d_tf = d["flops"] / (d["ms"] * 1e-3) / 1e12
            roof["dominant"] = {"kernel": d["kernel"], "launches_per_step": d["launches"], "avg_us": round(1e3 * d["ms"] / d["launches"], 2),
                                "flops_per_launch": round(d["flops"] / d["launches"]), "achieved": round(d_tf, 2), "unit": "TFLOP/s",
                                "frac": round(d_tf / PEAK_MFMA_TFLOPS, 4),
                                "source": "HIP event pairs around every launch of one eagerly launched serial forward (opd_detr_kernel_table); "
                                          "compare with the kernel's AverageNs in profiles/*_bench_streams1_kernel_stats.csv"}
            roof["kernels"] = [{"kernel": r["kernel"], "launches": r["launches"], "ms": round(r["ms"], 4), "gflop": round(r["flops"] / 1e9, 2)} for r in krows[:12]]
        if (B, H, W) == (8, 800, 1333) and args.arch == "r50":
            # achieved HBM GB/s of the convolution stages: SURVEY.md section 8(d)'s unfused per-layer minimum bytes of each stage (MB per
            # frame, bf16/fp16) x 8 frames / the stage's duration measured live with HIP events on the library's stream (profiling mode:
            # eager launches, so the few-us gaps between a stage's launches are included)
            stage_mb = {"stem+pool": 40.6, "stage1": 17.1 + 51.5 + 171.0 + 85.6, "stage2": 51.4 + 21.7 + 86.0 + 51.6 + 64.5 + 26.5,
                        "stage3": 25.9 + 11.9 + 67.7 + 26.8 + 56.4 + 27.4, "stage4": 14.0 + 10.1 + 22.4 + 17.1 + 15.0 + 13.7}
            roof["conv_stages_hbm"] = [
                {"stage": name, "ms": stage_ms[i], "algorithmic_GB": round(mb * B / 1e3, 3),   # stage_ms[0] = stem + pool, [1..4] = stages 1-4
                 "GB_per_s": round(mb * B / 1e3 / (stage_ms[i] * 1e-3), 1) if stage_ms[i] > 0 else None,
                 "frac_of_peak": round(mb * B / 1e3 / (stage_ms[i] * 1e-3) / PEAK_HBM_GBS, 3) if stage_ms[i] > 0 else None}
                for i, (name, mb) in enumerate(stage_mb.items())]
            # MFMA-pipe utilisation of the attention / linear kernels from the committed SQ counter pass of the same build
            sq_path = next((q for q in (os.path.join(ROOT, "profiles", n) for n in ("r05_pmc_sq.json", "r04_pmc_sq.json", "r03_pmc_sq.json")) if os.path.exists(q)), "")
            if sq_path:
                sq = json.load(open(sq_path))
                pick = lambda sub: {k: v["mfma_busy_pct"] for k, v in sq["kernels"].items() if sub in k}
                roof["mfma_busy_pct"] = {"source": f"committed profile, not measured in this run: profiles/{os.path.basename(sq_path)} (rocprofv3 --pmc SQ pass, one serial forward)",
                                         "whole_forward": sq["whole_forward_mfma_busy_pct"], "attention": pick("attention_kernel"),
                                         "row_owner_linears": pick("gemm_ln256"), "implicit_gemm": pick("conv_gemm_dma_kernel"),
                                         "fused_tails": {**pick("btail_kernel"), **pick("btail256_kernel")}}

    total_frames = B * world * args.steps
    fps = total_frames / elapsed
    if rank == 0:
        net = "101" if args.arch == "r101" else "50"
        out = {
            "metric": f"frames/sec (Phase-2 DETR detect) at {H}x{W} batch {B}",
            "value": round(fps, 2), "unit": "frames/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(1e3 * elapsed / args.steps, 3), "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": args.dtype, "data": "synthetic",
            "config": {"workload": f"facebook/detr-resnet-{net} architecture (seeded synthetic weights), batch {B} per GPU, "
                                   f"{H}x{W} uint8 BGR frames resident in HBM, forward + device post-process + records to host + person filter/NMS "
                                   "on the orchestrator; "
                                   + ("fp16 operands / fp32 accumulate (BASELINE configs[1] names bf16: same MFMA rate, fp16 keeps the 1e-3 box "
                                      "tolerance; --dtype bf16 runs that mode); " if args.dtype == "f16" else
                                      "bf16 operands / fp32 accumulate (OPD_FLAG_BF16, the type BASELINE configs[1] names; the decoder's linear layers on "
                                      "split fp16 operands as in the default mode); ")
                                   + ("blocking steps" if args.sync_steps else
                                      f"steps submitted asynchronously over {NS} detector handle(s), every step's records fetched to host")
                                   + ((", RCCL all-gather of detection records" if backend == "nccl" else f", {backend} REHEARSAL (ranks share device 0)")
                                      if world > 1 else ""),
                       "global_batch": B * world, "parallelism": f"frame-sharded dp{world}",
                       "batches_in_flight_per_gpu": 1 if args.sync_steps else NS},
            "roofline": roof,
            "serial": serial,
            "sustained": sustained,
            "stage_ms": stage_ms,   # inside the replayed graph of a single-stream handle (eager per-launch form: roofline.stage_ms_eager)
            "exchange": exchange,
            "detections_last_step": int(np.asarray(counts).clip(min=0).sum()) if counts is not None else None,
        }
        if dumped is not None:
            out["dump_outputs"] = dumped
        if rehearsal:
            out["rehearsal"] = "cpu: no device compute, not a measurement"
        if roof is not None and serial is not None and roof.get("graph_ms_per_step"):
            # the serial leg dissected: device time of its forward inside the graph (<= the step, which adds the records' way to the host
            # and the NMS), and the whole path's algorithmic FLOPs against it
            g_ms = roof["graph_ms_per_step"]
            rs = {"ms_per_step": serial["ms_per_step"], "graph_device_ms": g_ms, "closes": bool(g_ms <= serial["ms_per_step"])}
            if (H, W) == (800, 1333) and args.arch == "r50":
                tf = 203.2e9 * B / (g_ms * 1e-3) / 1e12
                rs.update({"bound": "mfma", "achieved": round(tf, 2), "peak": PEAK_MFMA_TFLOPS, "unit": "TFLOP/s", "frac": round(tf / PEAK_MFMA_TFLOPS, 4)})
            out["roofline_serial"] = rs
        if (H, W) == (800, 1333) and args.arch == "r50" and roof is not None:
            # SURVEY.md section 8(d) headline: the whole path's algorithmic FLOPs (203.2 GFLOP per r50 frame at 800x1333) x frames/s
            # per GPU against the dense MFMA peak; this one includes every gap, the attention, pre- and post-processing
            path_tf = 203.2e9 * fps / world / 1e12
            roof["whole_path"] = {"flops_per_frame": 203.2e9, "achieved": round(path_tf, 2), "frac": round(path_tf / PEAK_MFMA_TFLOPS, 4)}
        if world == 1 and not args.no_cpu_baseline and args.arch == "r50" and not rehearsal:
            out["cpu_baseline"] = cpu_baseline(path, H, W)
            out["speedup_vs_cpu_baseline"] = round(fps / out["cpu_baseline"]["value"], 1)
        print(json.dumps(out), file=json_out, flush=True)
    if world > 1:
        dist.barrier()   # every rank leaves together: rank 0's local legs above are over, and no rank tears its communicator down while a peer is still at work
    for cx in comms:
        lib.opd_comm_destroy(cx)
    for hx in handles:
        lib.opd_detr_destroy(hx)
    if world > 1:
        dist.destroy_process_group()
    return 0


if __name__ == "__main__":
    sys.exit(main())
