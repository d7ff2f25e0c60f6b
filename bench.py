"""Headline benchmark: images/sec @640x640, batch 32 per GPU, MSPA-C2f + GD-neck YOLOv8n (BASELINE.json configs[1]).

    python bench.py [--gpus N --steps K --warmup W] [--dtype bf16|f32] [--mode infer|train] [--full] [--dump-outputs DIR]

N > 1 without a launcher: this process starts `python -m torch.distributed.run --nproc-per-node N ... bench.py` as a CHILD before it
touches the GPU and exits with the child's code (one rank per GPU over RCCL); under torchrun the ranks read RANK / WORLD_SIZE.

mode infer (default, the headline): a step = one pass of the hot path over one resident batch: detection forward (all layers, HIP
kernels through the C ABI) + Detect decode + batched NMS (predict settings conf 0.25 / iou 0.7), replayed from a hipGraph.  R = 8
different batches (> 256 MiB together, so the Infinity Cache cannot hold the inputs) are resident in HBM before the timed region and
are cycled through, one hipGraph per batch.  Inference shards over the batch with no collective: N ranks = N replicas with disjoint
batches ("weak" scaling); the only collective is the MAX of the per-rank times.
mode train (BASELINE configs[2]): a step = DetectionTrainer.step on a resident uint8 batch with synthetic labels: train-mode forward,
fused assigner + loss, HIP reverse pass, bucketed RCCL all-reduce of the flat gradient buffer, clip + SGD + EMA.

Prints ONE JSON line on rank 0.  A plain run sets up, warms up, times the steps and prints the headline (`value`, `ms_per_step`); `roofline`,
`cpu_baseline` and `config.ms_per_step_one_batch_at_a_time` are null.  --full adds what takes runs of its own: the check of the batches in
flight against their serial replay and the one-batch-at-a-time latency, `roofline` (dominant kernel, HIP-event timed) and `cpu_baseline` (the
CPU oracle - a port of the reference's path - timed on the host cores with the protocol of SURVEY 8(d) / BASELINE.md section 3).
--dump-outputs DIR writes what the timed path returned in its last step as DIR/<name>.npy (float32 / float64): inference
`detections` [B, max_det, 6], `kept_anchor` [B, max_det] and `counts` [B] (rows past counts[i], which the kernel leaves unwritten, are
written as 0 / -1); training `loss`, `loss_items` and `params` (the flat fp32 parameter + buffer vector after the step, at most 4 M
elements: a fixed seeded sample of a larger model).  Inputs and weights are seeded, so the same arguments give the same inputs in every run.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0          # MI355X_MICROARCH.md: HBM3E peak (spec)
MFMA_PEAK_TFLOPS = {'bf16': 2500.0, 'f32': 157.3, 'fp8': 5000.0}   # fp8: the dtype's dense peak (block-scaled K=128 form); the non-scaled 16x16x32 e4m3 form used here runs at the bf16 rate
N_RESIDENT = 8                 # resident input batches cycled through (8 x 78.6 MB bf16 = 629 MB > the 256 MiB Infinity Cache)
DUMP_CAP = 1 << 22             # elements per array written by --dump-outputs (16 MB of fp32; the inference outputs are far smaller)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=1)
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--mode', choices=['infer', 'train'], default='infer')
    ap.add_argument('--batch', type=int, default=32, help='images per GPU')
    ap.add_argument('--imgsz', type=int, default=640)
    ap.add_argument('--inflight', type=int, default=None, help='S batches in flight: the resident batches\' graphs are replayed round-robin on S streams (inference; results are checked against serial replay)')
    ap.add_argument('--input', choices=['model', 'f32', 'u8'], default='model',
                    help="dtype of the resident image batch: 'model' = the compute dtype, what the reference's predictor hands its model "
                         "(img.half() / 255, engine/predictor.py:128-129); 'u8' = raw uint8, /255 fused into the stem kernel")
    ap.add_argument('--dtype', default='bf16', choices=['bf16', 'f32', 'fp8'],
                    help="fp8 (BASELINE configs[4], inference only): e4m3 operands on the implicit-GEMM convolutions (model.quantize_fp8 on one "
                         "calibration batch), bf16 activations in HBM and bf16 block kernels")
    ap.add_argument('--model', default='mspa_c2f_gd_yolov8')
    ap.add_argument('--scale', default='n')
    ap.add_argument('--no-graph', action='store_true')
    ap.add_argument('--no-cpu-baseline', action='store_true')
    ap.add_argument('--resident', type=int, default=N_RESIDENT)
    ap.add_argument('--full', action='store_true',
                    help='also run the serial-replay check and one-batch-at-a-time latency of the batches in flight, the roofline pass and the CPU baseline')
    ap.add_argument('--dump-outputs', metavar='DIR', default=None, help="write the timed path's outputs of its last step as DIR/<name>.npy")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error('--steps must be at least 1')
    return args


def dump_outputs(path, arrays):
    """name -> numpy array -> path/<name>.npy.  An array of more than DUMP_CAP elements is written as a sample of its flattened values at
    fixed seeded indices (the same in every run), which keeps the files of one run below 64 MB."""
    import numpy as np
    os.makedirs(path, exist_ok=True)
    for name, a in arrays.items():
        if a.size > DUMP_CAP:
            a = a.reshape(-1)[np.sort(np.random.default_rng(0).choice(a.size, DUMP_CAP, replace=False))]
        np.save(os.path.join(path, name + '.npy'), a)


def launch_ranks(args):
    """--gpus N > 1 and no launcher: start N fresh worker processes (torch.distributed.run) as a child; this parent never touches the GPU."""
    import socket
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', f'--nproc-per-node={args.gpus}', '--master-addr', '127.0.0.1',
           '--master-port', str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
    return subprocess.run(cmd, env=env).returncode


def host_cpu():
    model = 'unknown'
    try:
        for line in open('/proc/cpuinfo'):
            if line.startswith('model name'):
                model = line.split(':', 1)[1].strip()
                break
    except OSError:
        pass
    try:
        cores = len(os.sched_getaffinity(0))
    except AttributeError:
        cores = os.cpu_count() or 1
    return model, cores


def cpu_baseline(cfg, model, args):
    """The oracle (CPU port of the reference path, BN folded like AutoBackend(fuse=True)) timed with the protocol of SURVEY 8(d): batch 32,
    torch threads = the host cores this process may use, 3 warm-up + >= 10 timed iterations (time.perf_counter), forward-only and
    forward + NMS reported separately.  NMS = the reference's stages in numpy + the greedy kernel in C (the reference calls
    torchvision's compiled kernel there)."""
    import torch
    from mgdt_yolo_amd.seeding import seeded_images
    from oracle import layers as OL
    from oracle import nms as ON
    cpu_model, avail = host_cpu()
    # a 1-GPU box is granted a 16-core CPU share whatever the affinity mask says: more threads only thrash (override: MGDT_CPU_THREADS)
    cores = int(os.environ.get('MGDT_CPU_THREADS', min(avail, 16)))
    torch.set_num_threads(cores)
    sd = {k: v.detach().float().cpu().clone() for k, v in model.state_dict().items()}
    b = args.batch
    x = seeded_images(b, args.imgsz, args.imgsz, seed=0)
    strides = model.stride.tolist()

    def fwd():
        with torch.no_grad():
            return OL.model_forward(cfg, sd, x, strides, fused=True)[0]

    def nms(y):
        return ON.non_max_suppression(y.numpy(), conf_thres=0.25, iou_thres=0.7, compiled=True)

    def timed(warm, nmin, budget):
        for _ in range(warm):
            nms(fwd())
        t_f, t_n, reps = 0.0, 0.0, 0
        while reps < nmin and (reps < 3 or t_f + t_n < budget):
            t0 = time.perf_counter()
            y = fwd()
            t1 = time.perf_counter()
            nms(y)
            t2 = time.perf_counter()
            t_f += t1 - t0
            t_n += t2 - t1
            reps += 1
        return t_f, t_n, reps

    t_f, t_n, reps = timed(3, 10, float(os.environ.get('MGDT_CPU_BUDGET_S', 60)))
    out = {'value': round(b * reps / (t_f + t_n), 2), 'unit': 'images/sec', 'cores': cores, 'kind': 'port',
           'forward_only': round(b * reps / t_f, 2), 'forward_plus_nms': round(b * reps / (t_f + t_n), 2), 'cpu_model': cpu_model,
           'cores_available': avail,
           'sample': f'3 warm-up + {reps} timed x batch {b} @ {args.imgsz}x{args.imgsz}, torch-CPU fp32 oracle forward (BN folded), '
                     f'NMS conf 0.25 / iou 0.7 (numpy stages + C greedy kernel); value = forward + NMS'}
    if avail > cores and not os.environ.get('MGDT_CPU_SKIP_ALL_CORES'):
        # BASELINE.md section 3 asks for all physical host cores; `value` keeps the 1-GPU lease's 16-core share (what this process is
        # entitled to on a shared host).  The all-cores figure is reported beside it from a SMALL sample with a hard time bound: on a shared
        # box 256 threads of a 16-core share thrash (measured: 0.37 images/s), and the default bench run has to end within minutes.
        ab = min(b, 8)
        xa = x[:ab]
        torch.set_num_threads(avail)
        t0 = time.perf_counter()
        with torch.no_grad():
            OL.model_forward(cfg, sd, xa, strides, fused=True)
        warm = time.perf_counter() - t0
        if warm > 15.0:
            out['all_cores'] = {'cores': avail, 'value': None, 'note': f'skipped: one warm-up forward of {ab} images took {warm:.1f} s on {avail} threads '
                                                                       f'({ab / warm:.2f} images/s): this process is granted a {cores}-core share of the host'}
        else:
            t_a, n_a = 0.0, 0
            while n_a < 3 and t_a < 20.0:
                t0 = time.perf_counter()
                with torch.no_grad():
                    OL.model_forward(cfg, sd, xa, strides, fused=True)
                t_a += time.perf_counter() - t0
                n_a += 1
            out['all_cores'] = {'cores': avail, 'value': round(ab * n_a / t_a, 2), 'forward_only': round(ab * n_a / t_a, 2), 'sample': f'1 warm-up + {n_a} timed x batch {ab}, forward only'}
        torch.set_num_threads(cores)
    return out


def roofline_of(prof_rows, reps, step_ms, graph, args):
    """Dominant kernel family of the step from an instrumented eager pass (HIP-event pairs on the launch stream)."""
    agg = {}
    for name, meta, ms in prof_rows:
        key = (name, meta['shape'] if meta else None)
        a = agg.setdefault(key, [0.0, 0, meta])
        a[0] += ms
        a[1] += 1
    total_ms = sum(v[0] for v in agg.values()) / reps
    per_name, launches = {}, 0
    for (name, _), v in agg.items():
        per_name[name] = per_name.get(name, 0.0) + v[0] / reps
        launches += v[1] // reps
    # dominant kernel = the op with the largest share of the step; `achieved` = its algorithmic bytes (or flops) per launch / its average
    # launch duration, both averaged over all its launches of one step
    fam = {}
    for (name, shape), (ms, cnt, meta) in agg.items():
        if meta is None:
            continue
        f = fam.setdefault(name, {'ms': 0.0, 'n': 0, 'flops': 0.0, 'bytes': 0.0, 'shapes': []})
        f['ms'] += ms; f['n'] += cnt; f['flops'] += meta['flops'] * cnt; f['bytes'] += meta['bytes'] * cnt
        f['shapes'].append((ms / reps, cnt // reps, list(shape), meta))
    name, f = max(fam.items(), key=lambda kv: kv[1]['ms'])
    # two families are now within a few percent of each other (convolutions 0.29 ms, block kernels 0.28 ms of the eager step): run-to-run noise must not
    # flip the reported kernel, so the convolution family - the one the PMC traffic figure and every earlier round refer to - keeps the title while it is
    # within 5 % of the largest share
    for keep in ('conv2d_fwd', 'conv2d_fp8_fwd'):
        if keep in fam and fam[keep]['ms'] >= 0.95 * f['ms']:
            name, f = keep, fam[keep]
            break
    # eager launches start on an idle queue (Python issues slower than the GPU drains), which adds a ramp to every event pair; the graph
    # replay of the timed region has no such gaps.  Rescale the eager per-launch times so that they sum to the measured replay step.
    scale = step_ms / total_ms if graph else 1.0
    avg_eager_s = f['ms'] / f['n'] * 1e-3
    avg_s = avg_eager_s * scale
    flops_l, bytes_l = f['flops'] / f['n'], f['bytes'] / f['n']
    ai = flops_l / bytes_l
    ridge = MFMA_PEAK_TFLOPS[args.dtype] * 1e12 / (HBM_PEAK_GBS * 1e9)
    if ai >= ridge:
        ach = flops_l / avg_s / 1e12
        roof = {'bound': 'mfma', 'achieved': round(ach, 2), 'peak': MFMA_PEAK_TFLOPS[args.dtype], 'unit': 'TFLOP/s',
                'frac': round(ach / MFMA_PEAK_TFLOPS[args.dtype], 4)}
    else:
        ach = bytes_l / avg_s / 1e9
        roof = {'bound': 'hbm', 'achieved': round(ach, 1), 'peak': HBM_PEAK_GBS, 'unit': 'GB/s', 'frac': round(ach / HBM_PEAK_GBS, 4)}
    kern = {'conv2d_fp8_fwd': 'conv_igemm_kernel<.., Q8> (e4m3 MFMA)', 'conv2d_fwd': 'conv_igemm_kernel (+ conv3x3_lds_kernel for the 64->96 Detect-branch 3x3)', 'conv2d_direct_fwd': 'conv_stem_kernel', 'cnx_mlp_fwd': 'cnx_mlp_kernel<STATS> + cnx_mlp_kernel<APPLY>',
            'pw_chain3_fwd': 'pw_chain3_kernel', 'conv1x1_inject_fwd': 'conv1x1_inject_kernel', 'csp_block_fwd': 'csp_block_kernel',
            'cnx_block_fwd': 'cnx_block_kernel', 'conv1x1_inject_conv_fwd': 'conv1x1_inject_conv_kernel'}.get(name, name)
    traffic, tsrc, tat, tstale = None, None, None, None
    # the launches the PMC figure was averaged over, as a fingerprint: op name + every (shape, launches per step) of the family + the step's
    # launch count.  tools/pmc_summary.py stores the fingerprint of the run it measured; a different one here means the kernel set changed
    # since, and the stored traffic is NOT reported.
    import hashlib
    sig = hashlib.sha1(json.dumps([name, launches, sorted((list(sh), c) for _, c, sh, _ in f['shapes'])]).encode()).hexdigest()[:12]
    tfile = os.path.join(ROOT, 'profiles', 'pmc_traffic.json')     # rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes (tools/prof_pmc.sh), corrected
    if os.path.exists(tfile):
        ent = json.load(open(tfile)).get(f'{name}|{args.dtype}|b{args.batch}|{args.imgsz}')
        if ent and ent.get('launch_signature') == sig:
            traffic, tsrc, tat = ent['hbm_bytes_per_launch'], ent.get('source'), ent.get('measured_at')
        elif ent:
            tstale = f"profiles/pmc_traffic.json was measured at {ent.get('measured_at')} for launch set {ent.get('launch_signature')}, this run's is {sig}: not reported"
    top = sorted(f['shapes'], key=lambda t: -t[0])[:6]
    roof.update({'traffic': traffic, 'traffic_source': tsrc, 'traffic_measured_at': tat, 'traffic_stale': tstale, 'launch_signature': sig, 'kernel': f'{kern} ({name})', 'launches_per_step': f['n'] // reps,
                 'avg_us': round(avg_s * 1e6, 2), 'avg_us_eager_events': round(avg_eager_s * 1e6, 2), 'eager_to_replay_scale': round(scale, 4),
                 'flops_per_launch': round(flops_l), 'bytes_per_launch': round(bytes_l), 'arith_intensity': round(ai, 1),
                 'share_of_eager_step': round(f['ms'] / reps / total_ms, 3), 'all_launches_per_step': launches,
                 'largest_shapes_b_cin_h_w_cout_k_s': [{'shape': sh, 'launches': c, 'us_per_launch': round(ms_ / c * 1e3, 1),
                                                        'GBps': round(m['bytes'] / (ms_ / c * 1e-3) / 1e9), 'TFLOPs': round(m['flops'] / (ms_ / c * 1e-3) / 1e12, 1)}
                                                       for ms_, c, sh, m in top],
                 'eager_ms_per_step_by_op': {k: round(v, 3) for k, v in sorted(per_name.items(), key=lambda kv: -kv[1])},
                 'eager_ms_per_step': round(total_ms, 3)})
    return roof


def main():
    args = parse()
    if args.inflight is None:        # default: 4 batches in flight for the captured inference step (each step is still one whole batch: forward + NMS)
        args.inflight = 4 if (args.mode == 'infer' and not args.no_graph) else 1
    if args.inflight > 1 and (args.mode != 'infer' or args.no_graph):
        raise SystemExit('bench.py: --inflight applies to the captured inference step only')
    if args.gpus > 1 and 'WORLD_SIZE' not in os.environ:
        sys.exit(launch_ranks(args))

    import torch
    from mgdt_yolo_amd import parallel
    rank, local, world = parallel.env_rank()
    if world != args.gpus:
        print(f'bench.py: --gpus {args.gpus} but {world} rank(s) joined (WORLD_SIZE={world}): refusing to report a number', file=sys.stderr)
        sys.exit(2)
    torch.cuda.set_device(local)
    dev = torch.device('cuda', local)
    dist = None
    if world > 1:
        dist = parallel.init('nccl', dev)
        if dist.get_world_size() != args.gpus:
            sys.exit(2)

    from mgdt_yolo_amd import ops
    from mgdt_yolo_amd.models import get_config
    from mgdt_yolo_amd.nn.tasks import DetectionModel
    from mgdt_yolo_amd.seeding import seed_state_dict_, seeded_images, seeded_labels

    def barrier():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    if args.dtype == 'fp8' and args.mode != 'infer':
        raise SystemExit('bench.py: --dtype fp8 is an inference configuration (BASELINE configs[4])')
    tdt = torch.float32 if args.dtype == 'f32' else torch.bfloat16
    graph_used = False
    serial_ref = None                  # --full, batches in flight: what every captured graph gives on its own serial replay

    if args.mode == 'train':
        from mgdt_yolo_amd.yolo.engine.trainer import DetectionTrainer
        nc = 80
        cfg = get_config(args.model, args.scale, nc)
        model = seed_state_dict_(DetectionModel(cfg, verbose=False), 0).to(dev)
        # bf16: activations / activation gradients in bf16, fp32 masters.  Single rank: the step is captured in a hipGraph after the first optimizer step
        tr = DetectionTrainer(model, world_size=world, amp=args.dtype == 'bf16', graph=not args.no_graph)
        graph_used = tr.graph
        R = max(1, min(args.resident, 4))
        batches = []
        for r in range(R):
            lab = seeded_labels(args.batch, nc, seed=parallel.shard_seed(1000 + 17 * r, rank))
            img = (seeded_images(args.batch, args.imgsz, args.imgsz, seed=parallel.shard_seed(100 + 17 * r, rank)) * 255).round().clamp_(0, 255).to(torch.uint8)
            batches.append(dict(img=img.to(dev), **lab))
        it = [0]
        last = [None]                   # (loss * B, loss items) of the latest step

        def run():
            last[0] = tr.step(batches[it[0] % R])
            it[0] += 1

        def step_eager():               # instrumented pass: per-launch events need the launches themselves
            g, tr.graph = tr.graph, False
            try:
                run()
            finally:
                tr.graph = g
        x_desc = 'uint8 NCHW images resident in HBM (/255 fused into the stem), synthetic labels (1-20 boxes / image)'
        workload = (f'{args.model}-{args.scale} (nc=80) {args.imgsz}x{args.imgsz} TRAINING step, batch {args.batch}/GPU (global {world * args.batch}): '
                    'train-mode forward (batch-stat BN) + fused assigner/loss + HIP reverse pass + bucketed RCCL all-reduce of the flat gradient buffer '
                    '+ clip/SGD(nesterov)/EMA' + (('; whole step replayed as one hipGraph' if world == 1 else '; step replayed as two hipGraphs around the flat-gradient all-reduce') if graph_used else '') + '; BASELINE configs[2]')
        metric = f'images/sec @{args.imgsz}x{args.imgsz} bs={args.batch} per GPU, data-parallel training step'
        parallelism = f'dp{world} (batch-sharded, one flat-gradient all-reduce per step over RCCL/xGMI)' if world > 1 else 'dp1 (no collective)'
        n_det = None
    else:
        cfg = get_config(args.model, args.scale, 80)
        model = seed_state_dict_(DetectionModel(cfg, verbose=False), 0).eval().to(dev).set_compute_dtype(tdt)
        R = max(1, args.resident)
        xs = []
        for r in range(R):                                                   # resident in HBM, values in [0, 1], disjoint per rank and per slot
            x = seeded_images(args.batch, args.imgsz, args.imgsz, seed=parallel.shard_seed(100 + 17 * r, rank)).to(dev)
            if args.input == 'u8':
                x = (x * 255).round().clamp_(0, 255).to(torch.uint8)
            elif args.input == 'model':
                x = x.to(tdt)
            xs.append(x)
        fp8_note = ''
        if args.dtype == 'fp8':    # calibrate on a batch that is not one of the timed ones
            table = model.quantize_fp8(seeded_images(args.batch, args.imgsz, args.imgsz, seed=parallel.shard_seed(9000, rank)).to(dev).to(tdt))
            fp8_note = f'; fp8: {len(table)} implicit-GEMM convolutions on e4m3 MFMAs (per-tensor activation / per-channel weight scales), bf16 elsewhere; BASELINE configs[4]'

        def step(x):
            y, _ = model(x)
            return ops.nms(y, 0.25, 0.7, None, False, False, 300, 30000, 7680)

        def step_eager():
            return step(xs[0])

        S = max(1, min(args.inflight, R))                 # lanes: graph r belongs to lane r % S; the lanes' replays run concurrently on S streams
        with torch.no_grad():
            out = step(xs[0])                       # packs the weights, allocates
            torch.cuda.synchronize()
            graphs, outs = [], []
            if not args.no_graph:
                side = torch.cuda.Stream()
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):
                    for j in range(S):              # per-lane state (the block barrier words of mgdt_cnx_block_fwd) is created outside capture
                        with ops.lane(j):
                            for _ in range(2):
                                out = step(xs[0])
                torch.cuda.current_stream().wait_stream(side)
                torch.cuda.synchronize()
                # one lane (serial replay): the R graphs share one activation pool.  Several lanes: every graph owns its pool - graphs that share
                # one may only replay in capture order, and a graph captured earlier reuses, as scratch, the memory that holds a later graph's
                # outputs (the results are compared after the timed loop, whatever graph ran last)
                pools = [torch.cuda.graph_pool_handle() for _ in range(R if S > 1 else 1)]
                for r in range(R):
                    g = torch.cuda.CUDAGraph()
                    # several ranks: RCCL's watchdog thread may poll events while this thread captures - keep the capture's error mode thread-local
                    with ops.lane(r % S), torch.cuda.graph(g, pool=pools[r % len(pools)], **({'capture_error_mode': 'thread_local'} if world > 1 else {})):
                        outs.append(step(xs[r]))
                    graphs.append(g)
                out = outs[-1]
                graph_used = True
        it = [0]
        lanes = [torch.cuda.Stream() for _ in range(S)] if (graph_used and S > 1) else []
        if lanes:
            # what every graph must produce: its own serial replay (counts, detections and kept anchors of the valid rows)
            def snapshot():
                res = []
                for o in outs:
                    valid = torch.arange(o[1].shape[1], device=dev)[None, :] < o[2][:, None]
                    res.append((o[2].clone(), o[0][valid].clone(), o[1][valid].clone()))
                return res
            if args.full:
                for g in graphs:
                    g.replay()
                torch.cuda.synchronize()
                serial_ref = snapshot()

            def run():
                r = it[0] % R
                with torch.cuda.stream(lanes[r % S]):
                    graphs[r].replay()
                it[0] += 1
        elif graph_used:
            def run():
                graphs[it[0] % R].replay()
                it[0] += 1
        else:
            def run():
                nonlocal out
                with torch.no_grad():
                    out = step(xs[it[0] % R])
                it[0] += 1
        x_desc = f'{str(xs[0].dtype).replace("torch.", "")} NCHW images, {R} different batches resident in HBM ({R * xs[0].numel() * xs[0].element_size() / 2**20:.0f} MiB) cycled'
        workload = (f'{args.model}-{args.scale} (MSPA-C2f + GD neck + Detect, nc=80) {args.imgsz}x{args.imgsz} inference, batch {args.batch}/GPU: '
                    f'forward + decode + NMS(conf 0.25, iou 0.7), ' + ('hipGraph replay' if graph_used else 'eager launches')
                    + (f', {S} batches in flight (one captured graph per resident batch, replayed round-robin on {S} streams)' if lanes else '') + fp8_note)
        metric = f'images/sec @{args.imgsz}x{args.imgsz} bs={args.batch} per GPU, detection forward + NMS (whole job: {world} GPU(s))'
        parallelism = f'replicas x{world} (batch-sharded, no data-path collective)'

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        barrier()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            fn()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        barrier()
        return parallel.max_over_ranks(t1 - t0, dev)

    def last_outputs():
        """What the timed path returned in its last step, as numpy arrays (float32 / float64)."""
        if args.mode == 'train':
            total, items = (torch.as_tensor(t).detach().float().reshape(-1).cpu().numpy() for t in last[0])
            return {'loss': total, 'loss_items': items, 'params': tr.state.data.detach().cpu().numpy()}
        det, kept, counts = outs[(it[0] - 1) % R] if graph_used else out
        valid = torch.arange(det.shape[1], device=dev)[None, :] < counts[:, None]
        return {'detections': torch.where(valid[..., None], det, 0.0).cpu().numpy(),
                'kept_anchor': torch.where(valid, kept, -1).double().cpu().numpy(), 'counts': counts.double().cpu().numpy()}

    elapsed = timed(run)
    serial_ms = None
    if args.mode == 'infer':
        if serial_ref is not None:
            # the overlapped replays must have produced exactly what the serial replays did; if they did not (never observed since the library is
            # built without packed-fp32 VALU ops, profiles/r03_graph_replay_root_cause.txt) the number is thrown away and the serial replay is timed
            bad = [r for r, (got, ref) in enumerate(zip(snapshot(), serial_ref)) if not all(torch.equal(a, b) for a, b in zip(got, ref))]
            bad = int(parallel.max_over_ranks(float(len(bad)), dev)) + (1 if os.environ.get('MGDT_BENCH_FORCE_FALLBACK') else 0)    # (the env knob exercises the fallback path)

            def run_serial():
                graphs[it[0] % R].replay()
                it[0] += 1
            if bad:
                print(f'bench.py: {bad} batch(es) differ between concurrent and serial replay - timing the serial replay instead', file=sys.stderr)
                workload = workload.replace(f', {S} batches in flight (one captured graph per resident batch, replayed round-robin on {S} streams)', '')
                lanes, S = [], 1
                elapsed = timed(run_serial)
        n_det = int(out[2].sum().item())
    if args.dump_outputs and rank == 0:          # before anything else replays the graphs
        dump_outputs(args.dump_outputs, last_outputs())
    if serial_ref is not None and not bad:       # one batch at a time, for the latency side of the trade
        it[0] = 0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(2 * R):
            run_serial()
        torch.cuda.synchronize()
        serial_ms = (time.perf_counter() - t0) / (2 * R) * 1e3

    # ---- roofline of the dominant kernel: eager launches bracketed by HIP events on the launch stream
    # Per-kernel durations only mean something when kernels run one after the other: the instrumented pass uses ONE stream (no parallel branch),
    # and its event pairs are rescaled to the replay of a graph captured the same way - one batch, one stream - not to the overlapped timed region.
    roof = None
    if rank == 0 and args.full:
        reps = 3
        ref_ms = elapsed / args.steps * 1e3
        side_was = ops.SIDE_STREAM
        if args.mode == 'infer':
            ops.SIDE_STREAM = False
        try:
            if args.mode == 'infer' and graph_used and (lanes or side_was):
                with torch.no_grad():
                    step(xs[0])
                    torch.cuda.synchronize()
                    g1 = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(g1, **({'capture_error_mode': 'thread_local'} if world > 1 else {})):      # (RCCL's watchdog thread, as above)
                        o1 = step(xs[0])
                    for _ in range(3):
                        g1.replay()
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(20):
                        g1.replay()
                    torch.cuda.synchronize()
                    ref_ms = (time.perf_counter() - t0) / 20 * 1e3
                    del g1, o1
            with torch.no_grad() if args.mode == 'infer' else torch.enable_grad():
                with ops.profile() as prof:
                    for _ in range(reps):
                        step_eager()
        finally:
            ops.SIDE_STREAM = side_was
        roof = roofline_of(prof.rows, reps, ref_ms, graph_used, args)
        roof['single_stream_replay_ms'] = round(ref_ms, 4)

    if rank == 0:
        ms_step = elapsed / args.steps * 1e3
        value = parallel.aggregate_throughput(args.batch, args.steps, elapsed, world)
        line = {'metric': metric, 'value': round(value, 1), 'unit': 'images/sec',
                'n_gpus': world, 'steps': args.steps, 'warmup': args.warmup, 'ms_per_step': round(ms_step, 4), 'higher_is_better': True,
                'scaling': 'weak', 'vs_baseline': None, 'dtype': args.dtype, 'data': 'synthetic',
                'config': {'workload': workload, 'global_batch': world * args.batch, 'parallelism': parallelism, 'rccl_ranks': world,
                           'input': x_desc, 'detections_last_step': n_det, 'weights': 'seeded random init (no checkpoints offline)',
                           'timed_region_s': round(elapsed, 3), 'batches_in_flight': (S if args.mode == 'infer' and graph_used else 1),
                           'ms_per_step_one_batch_at_a_time': (round(serial_ms, 4) if serial_ms else None)},
                'roofline': roof}
        # whole-step fractions against SURVEY 8(d)'s layer-level algorithmic work per image (each top-level layer reads its inputs and writes
        # its output once, weights amortised; 2*MAC over every conv / linear): the distance of the WHOLE step - not of one kernel - from the chip
        per_img = {('mspa_c2f_gd_yolov8', 'n', 640): (22.04e6, 5.278e9), ('yolov8', 'n', 640): (23.21e6, 7.479e9)}.get((args.model, args.scale, args.imgsz))
        if per_img is not None and args.mode == 'infer' and roof is not None:
            esz = 4 if args.dtype == 'f32' else 2
            by, fl = per_img[0] * esz * args.batch, per_img[1] * args.batch
            roof['step_hbm_frac'] = round(by / (ms_step * 1e-3) / (HBM_PEAK_GBS * 1e9), 4)
            roof['step_mfma_frac'] = round(fl / (ms_step * 1e-3) / (MFMA_PEAK_TFLOPS[args.dtype] * 1e12), 4)
            roof['step_algorithmic'] = {'bytes_per_step': round(by), 'flops_per_step': round(fl), 'source': 'SURVEY.md 8(d): 22.04 M elements and 5.278 GFLOP per 640x640 image (layer granularity)'}
        if args.full and not args.no_cpu_baseline and world == 1 and args.mode == 'infer':
            line['cpu_baseline'] = cpu_baseline(cfg, model, args)
        else:
            line['cpu_baseline'] = None
        print(json.dumps(line))
    if world > 1:
        dist.destroy_process_group()


if __name__ == '__main__':
    main()
