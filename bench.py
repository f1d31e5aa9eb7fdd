#!/usr/bin/env python
"""bench.py -- headline benchmark of the MI355X speech-enhancement hot path.

Metric (BASELINE.json): enhanced 10 s utterances / second.  Workload at every N = configs[1]:
"TERA-base upstream + 2-layer mask head on libri-test-clean-10s, batch 32, bf16, 1 x MI355X", i.e. one
evaluate()-style pass (runner.py:556-575) per step over a batch of 32 synthetic 10 s / 16 kHz utterances
already resident in HBM:  STFT of the noisy + clean channels -> mel/log/delta/CMVN features -> 6-layer
768/12/3072 encoder (the only architecture config the reference ships, config/pretrain_sample.yaml:1-22)
-> TransformerSpecPredictionHead + exp/ReLU -> iSTFT with the noisy phase -> level normalisation to the
clean wav -> masked log-L1 loss.  Weights: seeded random at the real sizes (no checkpoints exist offline).

Multi-GPU: utterances shard data-parallel with NO data-path collective (inference); every rank runs
the same per-GPU batch ("weak" scaling); value = all utterances / max-over-ranks time.

    python bench.py --gpus 1 --steps 20 --warmup 3       set up, warm up, time the steps, print the line: nothing else runs
    python bench.py ... --full              + the side legs as extra keys of the line (roofline, host-fed, parity-mode rates, CPU baseline)
    python bench.py ... --dump-outputs DIR  + the last timed step's outputs as DIR/<name>.npy (same arguments -> same inputs, run to run)
    python bench.py --gpus N ...            (no torchrun environment: starts the N ranks itself, see launch_ranks())
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py --gpus N ...
Prints ONE JSON line on rank 0 (`n_gpus` = the world size the ranks OBSERVED through the collective, checked against --gpus).
"""
import argparse
import ctypes
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0          # MI355X_MICROARCH.md: HBM3E 8 TB/s
MFMA_BF16_PEAK_TFLOPS = 2500.0  # dense bf16


def cpu_baseline(batch, layers, seconds_budget=25.0):
    """The oracle (CPU restatement of the reference path) timed on this box's host cores, bounded sample."""
    import oracle
    from oracle import decode as odec, encoder as oenc, heads as oheads, objective as oobj, preprocessor as opre
    from speech_enhancement_by_s3prl_amd import pipeline, synth
    # threads actually used: this process's CPU share (affinity), capped at 16 -- the GPU box gives one GPU job a
    # 16-core share of a 256-thread host; asking torch for all 256 oversubscribes it by 16x
    try:
        cores = len(os.sched_getaffinity(0))
    except AttributeError:
        cores = os.cpu_count() or 1
    cores = max(1, min(cores, 16))
    torch.set_num_threads(cores)
    cfg = pipeline.make_config(layers=layers)
    ckpt = pipeline.synthetic_checkpoint(cfg, seed=0)
    ocfg = oenc.Config(cfg)
    geom = opre.Geometry()
    feat_list = [dict(cfg['online']['input'], channel=0), dict(pipeline.BASELINE_FEAT, channel=0),
                 opre.get_feat_config('linear', 0), opre.get_feat_config('phase', 0),
                 opre.get_feat_config('linear', 1), opre.get_feat_config('phase', 1)]
    lengths, wavs = synth.fast_batch(batch, 160000, seed=1)

    def one():
        with torch.no_grad():
            f = opre.forward(wavs, feat_list, geom)
            hid = oenc.encoder_forward(f[0], ckpt['Transformer'], ocfg, lengths=torch.full((batch,), f[0].shape[1]))
            pred, res = oheads.spec_head(hid, ckpt['SpecHead'], ocfg, log=True)
            wav = odec.decode_wav(pred, f[3], lengths, geom, wavs[:, 1])
            loss = oobj.l1(res['log_predicted'], f[4], odec.get_length_masks(lengths // 160 + 1))
        return wav, loss

    # protocol of BASELINE.md section 3: 3 warm-ups, >= 10 timed iterations where the budget allows (a bounded sample: 10-30 s of CPU work)
    t0 = time.perf_counter()
    one()
    warm = time.perf_counter() - t0
    n_warm = 3 if warm * 14 < seconds_budget * 1.5 else 1
    for _ in range(n_warm - 1):
        one()
    iters = max(3, min(10, int(seconds_budget / max(warm, 1e-3)) - n_warm))
    t0 = time.perf_counter()
    for _ in range(iters):
        one()
    dt = (time.perf_counter() - t0) / iters
    cpu_name = ''
    try:
        with open('/proc/cpuinfo') as fh:
            for line in fh:
                if line.startswith('model name'):
                    cpu_name = line.split(':', 1)[1].strip()
                    break
    except OSError:
        pass
    return {'value': batch / dt, 'unit': 'utt/s', 'cores': cores, 'kind': 'port',
            'sample': f'{n_warm} warm-ups + {iters} timed x batch of {batch} synthetic 10 s utterances, same pass (fp32 torch CPU oracle, L={layers}), '
                      f'{dt:.2f} s per batch on {cpu_name}'}


# committed counter passes (tools/collect_profiles.sh), one file per workload: bench.py cannot run counter passes on itself
PMC_FILES = {'enhance': 'r05c_pmc_fetch_write.json', 'finetune': 'r05c_finetune_pmc_fetch_write.json',
             'head:mel120': 'r05c_head_mel120_pmc_fetch_write.json', 'head:linear201': 'r05c_head_linear201_pmc_fetch_write.json'}


# every kernel the prof family 'gemm_bf16' times (csrc/gemm*.hip): the traffic figure is the launch-weighted mean over the same launches
GEMM_KERNELS = ('gemm2_bf16_kernel', 'gemm3_bf16_kernel', 'gemm4_res_ln_kernel', 'gemm6_bf16_kernel', 'gemm6p_bf16_kernel', 'gemm7_res_ln_kernel',
                'gemm8_res24_ln_kernel', 'gemm5_bf16_kernel')


def pmc_traffic(substrings, which='enhance'):
    """HBM bytes per launch of a kernel family from the committed rocprofv3 PMC passes of this same command (separate
    `--pmc FETCH_SIZE` / `--pmc WRITE_SIZE` runs, KB per dispatch; bench.py cannot run counter passes on itself).
    gfx950 correction (MI355X_MICROARCH.md, HBM / rocprofv3): FETCH_SIZE tallies 128-B requests at 64 B for 16-B-per-lane
    streams, so it is doubled; WRITE_SIZE is exact.  Returns None when the file is absent."""
    try:
        with open(os.path.join(ROOT, 'profiles', PMC_FILES[which])) as fh:
            d = json.load(fh)
    except (OSError, ValueError, KeyError):
        return None
    tot, n = 0.0, 0
    for name, v in d.items():
        if any(sub in name for sub in substrings) and 'FETCH_SIZE_KB_mean' in v and 'WRITE_SIZE_KB_mean' in v:
            tot += (2.0 * v['FETCH_SIZE_KB_mean'] + v['WRITE_SIZE_KB_mean']) * 1024.0 * v['launches']
            n += v['launches']
    return tot / n if n else None


def launch_ranks(n, argv):
    """`python bench.py --gpus N` outside torchrun: start N ranks as a CHILD `python -m torch.distributed.run` (this process has not
    touched the GPU and never execs), relay rank 0's JSON line and the child's exit code."""
    import socket
    import subprocess
    with socket.socket() as sock:
        sock.bind(('127.0.0.1', 0))
        port = sock.getsockname()[1]
    env = dict(os.environ)
    env.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', f'--nproc-per-node={n}', '--master-addr', '127.0.0.1',
           '--master-port', str(port), os.path.abspath(__file__)] + argv
    proc = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True)
    line = None
    for ln in proc.stdout.splitlines():
        if ln.startswith('{') and '"metric"' in ln:
            line = ln
        else:
            print(ln, file=sys.stderr)
    if proc.returncode != 0 or line is None:
        print(f'bench.py: the {n}-rank child exited with code {proc.returncode}' + ('' if line else ' and printed no JSON line'), file=sys.stderr)
        sys.exit(proc.returncode or 1)
    got = json.loads(line).get('n_gpus')
    if got != n:
        print(f'bench.py: asked for {n} ranks, the job observed {got}', file=sys.stderr)
        sys.exit(1)
    print(line, flush=True)
    sys.exit(0)


def launch_check(args):
    """--launch-check: the rank plumbing alone (process group, barrier, rank count by all-reduce, one JSON line), no kernels --
    what the CPU test of the launcher runs over gloo."""
    import torch.distributed as dist
    os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
    os.environ.setdefault('MASTER_PORT', '29500')
    os.environ.setdefault('RANK', '0')
    os.environ.setdefault('WORLD_SIZE', '1')
    dist.init_process_group(args.backend)
    dist.barrier()
    ones = torch.ones(1, dtype=torch.float64)
    dist.all_reduce(ones)
    world = int(ones.item())
    rank = dist.get_rank()
    dist.barrier()
    dist.destroy_process_group()
    if world != args.gpus:
        print(f'bench.py: --gpus {args.gpus} but {world} ranks joined', file=sys.stderr)
        sys.exit(1)
    if rank == 0:
        print(json.dumps({'metric': 'launch-check', 'n_gpus': world, 'world_observed': world, 'backend': args.backend}), flush=True)


def cpu_baseline_head(batch, head_feat, seconds_budget=20.0):
    """The oracle's restatement of the head pass (configs[3] / configs[0]) timed on this box's host cores, bounded sample."""
    from oracle import decode as odec, heads as oheads, objective as oobj, preprocessor as opre
    from speech_enhancement_by_s3prl_amd import synth
    try:
        cores = len(os.sched_getaffinity(0))
    except AttributeError:
        cores = os.cpu_count() or 1
    cores = max(1, min(cores, 16))
    torch.set_num_threads(cores)
    geom = opre.Geometry()
    feat = HEAD_FEATS[head_feat]
    feat_list = [dict(feat, channel=0), dict(feat, channel=0), opre.get_feat_config('linear', 0), opre.get_feat_config('phase', 0),
                 opre.get_feat_config('linear', 1), opre.get_feat_config('phase', 1)]
    lengths, wavs = synth.fast_batch(batch, 160000, seed=1)
    wavs = wavs[:, :2].contiguous()
    D = 120 if head_feat == 'mel120' else 201
    g = torch.Generator().manual_seed(0)
    W, b = torch.randn(201, D, generator=g) * 0.05, torch.randn(201, generator=g) * 0.05

    def one():
        with torch.no_grad():
            f = opre.forward(wavs, feat_list, geom)
            pred, _ = oheads.linear_residual(f[1], f[2], W, b)
            wav = odec.decode_wav(pred, f[3], lengths, geom, wavs[:, 1])
            loss = oobj.sisdr_objective(pred, f[4], odec.get_length_masks(lengths // 160 + 1))
        return wav, loss

    t0 = time.perf_counter()
    one()
    warm = time.perf_counter() - t0
    for _ in range(2):
        one()
    iters = max(3, min(10, int(seconds_budget / max(warm, 1e-3)) - 3))
    t0 = time.perf_counter()
    for _ in range(iters):
        one()
    dt = (time.perf_counter() - t0) / iters
    return {'value': batch / dt, 'unit': 'utt/s', 'cores': cores, 'kind': 'port',
            'sample': f'3 warm-ups + {iters} timed x batch of {batch} synthetic 10 s two-channel utterances, same pass (fp32 torch CPU oracle: torch.stft, '
                      f'features, LinearResidual, torch.istft, dB-norm, SISDR), {dt:.2f} s per batch'}


def extras_leg(args, w, dev, out):
    """extra keys of the line, never `value` (rank 0, after the process group is gone)"""
    from speech_enhancement_by_s3prl_amd import synth

    def rate(step, batch, steps, warm=2):
        lengths, wavs = synth.fast_batch(batch, 160000, seed=2000, device=dev)
        if args.workload == 'head':
            wavs = wavs[:, :2].contiguous()
        for _ in range(warm):
            step(wavs, lengths, w['max_len'])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            step(wavs, lengths, w['max_len'])
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / steps
        return {'value': batch / dt, 'unit': 'utt/s', 'ms_per_step': 1000.0 * dt, 'batch': batch}

    if args.workload == 'enhance' and args.streams == 1 and not args.graph:
        # the mode that meets north_star's 1e-4 on enhanced magnitudes (tests/test_gpu_encoder_fp32.py): exact-fp32 encoder + spec head
        up = w['upstream']
        up.set_precision('fp32')
        try:
            r = rate(w['step'], 8, 3, warm=1)
        finally:
            up.set_precision('bf16')
        r['note'] = ("TRANSFORMER.set_precision('fp32'): fp32 operands / products / sums on v_mfma_f32_32x32x2_f32 (1/16 of the bf16 matrix rate), the rate at "
                     'which the stated 1e-4 tolerance holds; not the headline value')
        out['fp32_parity_mode'] = r
        # the same tolerance on the bf16 matrix pipe: every nn.Linear as one bf16 GEMM over three-term operand splits, flash attention on two-term splits
        up.set_precision('bf16x3')
        try:
            r3 = rate(w['step'], 8, 5, warm=1)
            r3b = rate(w['step'], args.batch, 3, warm=1) if args.batch != 8 else None
        finally:
            up.set_precision('bf16')
        r3['note'] = ("TRANSFORMER.set_precision('bf16x3'): x1 w1 + x1 w2 + x2 w1 of the bf16 splits x = x1 + x2 (+ 2^-17) as ONE GEMM of depth 3 K per "
                      "nn.Linear, every producer writing the next operand's split itself (se_gemm_x3out_bf16, se_layernorm_x3_f32, se_mhsa_fwd_x3_split_f32; from 160 "
                      'row tiles on the N = 768 projections as one row-complete GEMM + residual + LayerNorm + split launch, se_gemm_res_ln_x3_bf16), attention as a '
                      'flash kernel on two-term splits of Q, K, V, P with an exact fp32 online softmax; meets the same 1e-4 test (tests/test_gpu_encoder_fp32.py: '
                      'enhanced magnitudes 7e-6); not the headline value')
        if r3b is not None:
            r3['at_bench_batch'] = r3b
        out['bf16x3_parity_mode'] = r3
    if args.workload == 'head' and not args.graph:
        r = rate(w['step'], 12, 50, warm=5)
        r['note'] = 'vcb.yaml:3 eval_batch_size = 12: launch-latency regime (one pass is ~10 launches of a few microseconds of work each)'
        out['batch_12'] = r
        try:      # the same pass replayed as ONE hipGraph (pipeline.GraphedStep): what the launch-latency regime gains from it
            from speech_enhancement_by_s3prl_amd import pipeline
            lengths, wavs = synth.fast_batch(12, 160000, seed=2000, device=dev)
            wavs = wavs[:, :2].contiguous()
            graphed = pipeline.GraphedStep(w['step'], wavs, lengths, w['max_len'])
            for _ in range(5):
                graphed(wavs, lengths)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(50):
                graphed(wavs, lengths)
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) / 50
            out['batch_12_graph'] = {'value': 12 / dt, 'unit': 'utt/s', 'ms_per_step': 1000.0 * dt, 'batch': 12,
                                     'note': 'the batch-12 pass captured once and replayed as one hipGraph (bench.py --graph does the same for `value`)'}
        except Exception as e:      # a side measurement must never take the line down
            out['batch_12_graph'] = {'error': repr(e)[:200]}


class Ranks:
    """The process group's lifetime.  Everything that may run a collective happens between __init__ and teardown(), in the SAME
    order on every rank (no `if rank == 0` around a step); the rank-0-only side legs (host-fed rate, CPU baseline, printing) run
    after teardown(), when no process group exists any more -- a rank cannot wait in a collective for a peer that is busy elsewhere."""

    def __init__(self, args):
        self.rank = int(os.environ.get('RANK', '0'))
        self.local_rank = int(os.environ.get('LOCAL_RANK', '0'))
        self.world = int(os.environ.get('WORLD_SIZE', '1'))
        self.distributed = self.world > 1 or 'RANK' in os.environ      # under torchrun always go through RCCL (also at N = 1)
        self.backend = args.backend
        if self.world != args.gpus:
            print(f'bench.py: --gpus {args.gpus} but WORLD_SIZE={self.world}', file=sys.stderr)
            sys.exit(2)
        self.stub = args.stub_step
        if self.stub:
            self.dev = torch.device('cpu')
        else:
            if not torch.cuda.is_available():
                print('bench.py needs an MI355X: the hot path has no CPU fallback', file=sys.stderr)
                sys.exit(2)
            if args.one_device:
                self.local_rank = 0
            torch.cuda.set_device(self.local_rank)
            self.dev = torch.device('cuda', self.local_rank)
        self.world_observed = 1
        if self.distributed:
            import torch.distributed as dist
            self.dist = dist
            os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
            os.environ.setdefault('MASTER_PORT', '29500')
            if self.stub:
                dist.init_process_group(args.backend)
            else:
                dist.init_process_group(args.backend, device_id=self.dev)
            dist.barrier()                      # creates the communicator now (not inside the timed region)
            ones = torch.ones(1, device=self.dev, dtype=torch.float64)
            dist.all_reduce(ones)               # the world size the collective itself sees
            self.world_observed = int(ones.item())
            if self.world_observed != args.gpus:
                print(f'bench.py: --gpus {args.gpus} but the all-reduce counted {self.world_observed} ranks', file=sys.stderr)
                sys.exit(2)

    def sync(self):
        if self.dev.type == 'cuda':
            torch.cuda.synchronize()
        if self.distributed:
            self.dist.barrier()
            if self.dev.type == 'cuda':
                torch.cuda.synchronize()

    def local_sync(self):
        if self.dev.type == 'cuda':
            torch.cuda.synchronize()

    def max_over_ranks(self, x):
        if not self.distributed:
            return x
        t = torch.tensor([x], device=self.dev, dtype=torch.float64)
        self.dist.all_reduce(t, op=self.dist.ReduceOp.MAX)
        return t.item()

    def teardown(self):
        """The LAST collective of the job, reached by every rank after the same sequence of collectives."""
        if self.distributed:
            self.dist.barrier()
            self.dist.destroy_process_group()
            self.distributed = False


HEAD_FEATS = {
    # SURVEY 8d's restatement of configs[3] ("same as config 1 but on GPU"): pseudo_noise.yaml's baseline features, 120 dims
    'mel120': {'feat_type': 'mel', 'log': True, 'delta': 2, 'cmvn': False},
    # vcb.yaml:10-14 literally: the linear power spectrogram itself is the head's input, 201 dims
    'linear201': {'feat_type': 'linear', 'log': False, 'delta': 0, 'cmvn': False},
}


def build_workload(args, ranks):
    """-> dict(step=callable(wavs, lengths, max_len) -> (wav_pred, loss, aux), wavs, lengths, max_len, collective, lib, describe)"""
    from speech_enhancement_by_s3prl_amd import _lib, pipeline, synth
    dev, rank = ranks.dev, ranks.rank
    lib = _lib.load()
    cfg = pipeline.make_config(layers=args.layers)
    w = {'lib': lib, 'collective': False, 'max_len': 160000, 'dtype': 'bf16'}
    lengths, wavs = synth.fast_batch(args.batch, 160000, seed=1000 + rank, device=dev)   # resident in HBM before timing
    if args.workload == 'head':
        from speech_enhancement_by_s3prl_amd.heads import LinearResidual
        from speech_enhancement_by_s3prl_amd.objective import SISDR
        feat = HEAD_FEATS[args.head_feat]
        pre = pipeline.build_preprocessor(cfg, dev, channel_inp=0, channel_tar=1, downstream_feat=feat, upstream='baseline')      # --upstream baseline
        torch.manual_seed(0)
        D = 120 if args.head_feat == 'mel120' else 201
        head = LinearResidual(input_size=D, output_size=201, cmvn=True).to(dev)
        hs = pipeline.HeadEnhanceStep(pre, head, criterion=SISDR())
        wavs = wavs[:, :2].contiguous()          # NoisyCleanDataset batches are (B, 2, T) = (noisy, clean): dataset.py:245, vcb.yaml:5-7

        def step(wavs, lengths, max_len):
            wav_pred, predicted, lin_tar, loss = hs(wavs, lengths, max_len=max_len)
            return wav_pred, loss, predicted
        w.update(step=step, pre=pre, dtype='f32')
    elif args.workload == 'enhance':
        ckpt = pipeline.synthetic_checkpoint(cfg, seed=0)
        upstream = pipeline.build_upstream(ckpt, dev)
        pre = pipeline.build_preprocessor(cfg, dev)
        w.update(step=pipeline.UpstreamEnhanceStep(pre, upstream, streams=args.streams), pre=pre, upstream=upstream)
    elif args.workload == 'finetune':
        import warnings
        warnings.simplefilter('ignore')
        from speech_enhancement_by_s3prl_amd.solver import get_optimizer
        ckpt = pipeline.synthetic_checkpoint(cfg, seed=0)
        pre = pipeline.build_preprocessor(cfg, dev)
        model = pipeline.build_mockingjay(ckpt, dev)
        opt = get_optimizer(list(model.named_parameters()), lr=4e-5, warmup_proportion=0.07, training_steps=100000)
        ft = pipeline.MockingjayFinetuneStep(pre, model, opt)        # broadcasts the parameters: a collective, on every rank

        def step(wavs, lengths, max_len):          # same call shape as the enhance step
            loss, gn, skipped = ft(wavs, lengths)
            return loss.reshape(1), loss, None
        w.update(step=step, pre=pre, collective=True)
    elif args.workload == 'lstm':
        from speech_enhancement_by_s3prl_amd.lstm import LSTM
        from speech_enhancement_by_s3prl_amd.solver import get_optimizer
        pre = pipeline.build_preprocessor(cfg, dev)
        head = LSTM(input_size=120, output_size=201, hidden_size=256, num_layers=3, bidirectional=True).to(dev)
        opt = get_optimizer(list(head.named_parameters()), lr=4e-5, warmup_proportion=0.07, training_steps=100000)
        ht = pipeline.HeadFinetuneStep(pre, head, opt)

        def step(wavs, lengths, max_len):
            loss, gn, skipped = ht(wavs, lengths)
            return loss.reshape(1), loss, None
        w.update(step=step, pre=pre, collective=True)
    w.update(wavs=wavs, lengths=lengths)
    if args.graph and args.workload in ('enhance', 'head'):
        graphed = pipeline.GraphedStep(w['step'], wavs, lengths, w['max_len'])
        w['step'] = lambda wavs, lengths, max_len: graphed(wavs, lengths)
    return w


def build_stub_workload(args, ranks):
    """--stub-step: the SAME control flow and the SAME collective sequence per step as the real workloads, on CPU tensors over gloo, with
    the HIP kernels replaced by a few torch lines: what tests/test_dist_gloo.py runs so that the driver's 8-GPU job is never the first
    execution of this file's N > 1 path.  The training stubs go through the product's own dist.py classes (global-mean criterion sums,
    BucketedGradSink's async per-layer all-reduces, FlatGradAllReducer's tail reduce + wait, clip, step)."""
    from speech_enhancement_by_s3prl_amd import dist as sdist
    g = torch.Generator().manual_seed(7 + ranks.rank)
    B, F, D, N = args.batch, 16, 12, 9
    feats = torch.randn(B, F, D, generator=g)
    tar = torch.rand(B, F, N, generator=g) + 0.1
    lens = torch.randint(1, F + 1, (B,), generator=g)
    w = {'lib': None, 'collective': args.workload in ('finetune', 'lstm'), 'max_len': F, 'wavs': feats, 'lengths': lens, 'dtype': 'f32'}
    if not w['collective']:
        torch.manual_seed(0)
        lin = torch.nn.Linear(D, N)

        def step(feats, lens, max_len):
            with torch.no_grad():
                out = lin(feats)
            return out, out.abs().mean(), None
        w['step'] = step
        return w
    torch.manual_seed(0)
    layers = torch.nn.ModuleList([torch.nn.Linear(D, D) for _ in range(3)] + [torch.nn.Linear(D, N)])
    sdist.broadcast_parameters(layers)
    params = list(layers.parameters())
    red = sdist.FlatGradAllReducer(params)
    sink = sdist.BucketedGradSink(red)
    opt = torch.optim.SGD(params, lr=1e-3)

    def step(feats, lens, max_len):
        x = feats
        for l in layers[:-1]:
            x = torch.tanh(l(x))
        logp = layers[-1](x)
        mask = (torch.arange(F)[None] < lens[:, None]).float()[..., None]
        s = ((logp - tar.log()).abs() * mask).sum()
        sums = sdist.all_reduce_sums(torch.stack([s.detach().double(), (mask.sum() * N).double()]))      # (sum, count) BEFORE dividing
        loss = s / sums[1].float()
        opt.zero_grad()
        loss.backward()
        sink.begin()
        for l in reversed(layers[:-1]):          # the encoder backward's per-layer callback, last layer first
            for p in l.parameters():
                sink.view(p).copy_(p.grad)
            sink.bucket_done(list(l.parameters()))
        flat = red.reduce(copy_back=True, sink=sink)     # the rest (the head) + wait for the bucket handles
        gn = float(torch.nn.utils.clip_grad_norm_(params, 1.0))
        if not (gn != gn or gn == float('inf')):
            opt.step()
        return flat[:1], (sums[0] / sums[1]).float(), None
    w['step'] = step
    return w


def roofline_report(args, lib, out):
    """reads the in-library HIP-event timings of the roofline leg (recorded on the launch stream around every kernel of the dominant families)"""
    fam = {}
    for kind, name in ((0, 'gemm_bf16'), (1, 'mhsa_fwd'), (2, 'stft'), (3, 'istft'), (5, 'head'), (6, 'mhsa_bwd')):
        ms, work, n = ctypes.c_double(), ctypes.c_double(), ctypes.c_longlong()
        lib.se_prof_read(kind, ctypes.byref(ms), ctypes.byref(work), ctypes.byref(n))
        fam[name] = (ms.value, work.value, n.value)
    others = {}

    def hbm_entry(name):
        ms, byts, n = fam[name]
        if ms <= 0:
            return None
        a = byts / (ms * 1e-3) / 1e9
        return {'bound': 'hbm', 'achieved': a, 'peak': HBM_PEAK_GBS, 'unit': 'GB/s', 'frac': a / HBM_PEAK_GBS, 'avg_launch_ms': ms / n,
                'launches': n, 'algorithmic_bytes_per_launch': byts / n, 'share_of_step_ms': ms / args.steps}

    def mfma_entry(name):
        ms, flop, n = fam[name]
        if ms <= 0:
            return None
        a = flop / (ms * 1e-3) / 1e12
        return {'bound': 'mfma', 'achieved': a, 'peak': MFMA_BF16_PEAK_TFLOPS, 'unit': 'TFLOP/s', 'frac': a / MFMA_BF16_PEAK_TFLOPS,
                'avg_launch_ms': ms / n, 'share_of_step_ms': ms / args.steps}

    if args.workload == 'head':
        # HBM-bound pass: the dominant kernel is the two-channel STFT launch
        e = hbm_entry('stft') or {}
        which = 'head:' + args.head_feat
        traffic = pmc_traffic(('se::stft_kernel', 'se::stft_small_kernel'), which) if args.batch == 256 and not args.graph else None
        out['roofline'] = dict(e, kernel='stft_kernel', traffic=traffic,
                               traffic_unit='HBM bytes per launch (2 x FETCH_SIZE + WRITE_SIZE, committed PMC passes: profiles/' + PMC_FILES[which] + ')')
        for name in ('istft', 'head'):
            e = hbm_entry(name)
            if e:
                others[name + '_kernel'] = e
        out['roofline_other_kernels'] = others
        return
    g_ms, g_flop, g_n = fam['gemm_bf16']
    achieved = g_flop / (g_ms * 1e-3) / 1e12 if g_ms > 0 else 0.0
    # the committed PMC passes are of the default command: report them only when this run is that command
    pmc_matches = (args.workload in ('enhance', 'finetune') and args.batch == 32 and args.layers == 6 and args.streams == 1 and not args.graph)
    traffic = pmc_traffic(GEMM_KERNELS, args.workload) if pmc_matches else None
    out['roofline'] = {'bound': 'mfma', 'kernel': 'gemm_bf16_kernel', 'achieved': achieved, 'peak': MFMA_BF16_PEAK_TFLOPS,
                       'unit': 'TFLOP/s', 'frac': achieved / MFMA_BF16_PEAK_TFLOPS, 'traffic': traffic,
                       'traffic_unit': 'HBM bytes per launch (2 x FETCH_SIZE + WRITE_SIZE, committed PMC passes: profiles/' + PMC_FILES.get(args.workload, '-') +
                                       '); counts L2 misses incl. Infinity-Cache hits: ~1.45x the algorithmic bytes of these launches',
                       'launches': g_n, 'avg_launch_ms': g_ms / max(g_n, 1),
                       'algorithmic_flop_per_launch': g_flop / max(g_n, 1)}
    for name, key in (('mhsa_fwd', 'mhsa_fwd_kernel'), ('mhsa_bwd', 'mhsa_bwd_kernels')):
        e = mfma_entry(name)
        if e:
            others[key] = e
    for name in ('stft', 'istft'):
        e = hbm_entry(name)
        if e:
            others[name + '_kernel'] = e
    others['gemm_share_of_step_ms'] = g_ms / args.steps
    out['roofline_other_kernels'] = others


def host_fed_leg(args, w, dev):
    """PCIe-inclusive side measurement (never `value`): the same K steps with every batch arriving from pinned HOST memory through the
    double-buffered feeder (feeder.py; the reference copies synchronously on the compute stream, runner.py:431-432, 556-557)"""
    from speech_enhancement_by_s3prl_amd.feeder import HostBatchFeeder
    step, max_len = w['step'], w['max_len']
    host_l, host_w = w['lengths'].cpu().pin_memory(), w['wavs'].cpu().pin_memory()

    def timed(channels):
        feeder = HostBatchFeeder([(host_l, host_w)] * args.warmup, dev, channels=channels)
        for dl, dw in feeder:
            step(dw, dl, max_len)
        torch.cuda.synchronize()
        feeder.batches = [(host_l, host_w)] * args.steps          # same slots: device buffers are allocated once, as in a real loop
        t0 = time.perf_counter()
        for dl, dw in feeder:
            step(dw, dl, max_len)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    el = timed(None)
    rec = {'value': args.batch * args.steps / el, 'unit': 'utt/s', 'ms_per_step': 1000.0 * el / args.steps,
           'bytes_per_step': host_w.numel() * 4 + host_l.numel() * 8,
           'note': 'rank 0 only, after the process group is gone; batches DMA-ed from pinned host memory on a copy stream, double buffered '
                   '(PCIe-inclusive; not the headline value)'}
    if host_w.shape[1] > 2:
        # the same with only the channels the pass reads (0 = noisy, 1 = clean; runner.py:558-561) crossing PCIe
        el = timed(2)
        rec['two_channels'] = {'value': args.batch * args.steps / el, 'ms_per_step': 1000.0 * el / args.steps,
                               'bytes_per_step': host_w.numel() * 4 * 2 // host_w.shape[1] + host_l.numel() * 8}
    return rec


DUMP_BUDGET_BYTES = 60 * 1000 * 1000      # --dump-outputs: all files together stay under 64 MB


def snapshot_outputs(named):
    """Host float32 copies of what the last timed step returned (taken before anything else runs the step again)."""
    return {name: t.detach().to('cpu', torch.float32).numpy().copy() for name, t in named if torch.is_tensor(t)}


def dump_outputs(dirname, arrays):
    """--dump-outputs: DIR/<name>.npy per output of the timed path.  An array above its share of the budget is written as a fixed sample:
    the flattened elements at the sorted indices numpy's default_rng(0) draws without replacement (the same indices in every run and build)."""
    import numpy as np
    os.makedirs(dirname, exist_ok=True)
    share = DUMP_BUDGET_BYTES // max(len(arrays), 1)
    if sum(a.nbytes for a in arrays.values()) <= DUMP_BUDGET_BYTES:
        share = DUMP_BUDGET_BYTES
    for name, a in arrays.items():
        if a.nbytes > share:
            idx = np.sort(np.random.default_rng(0).choice(a.size, share // a.itemsize, replace=False))
            a = a.reshape(-1)[idx]
        np.save(os.path.join(dirname, name + '.npy'), a)


def head_pass_bytes(head_feat):
    """algorithmic HBM bytes per utterance of the head pass: the sum over its kernels, and the fully fused bound"""
    T, F, K = 160000, 1001, 201
    D = 120 if head_feat == 'mel120' else 201
    stft = 2 * (4 * T + 2 * 4 * F * K)                       # both channels, power + phase each (2 249 608 B per utterance-channel)
    feats = (4 * F * 40 + 4 * F * D) if head_feat == 'mel120' else 0      # round 5: one pass, mel plane in, time-major rows out (was in + 3 x out)
    head = 4 * F * (D + 2 * K + K)                           # features + noisy power + clean power (the criterion's sums ride in the epilogue) in, predicted out
    istft = 2 * 4 * F * K + 4 * T + 4 * T                    # + the reference wav read by the level normalisation
    crit = 0                                                 # round 5: no pass of its own (was predicted + clean power: 2 x 4 F K)
    return {'sum_of_kernels': stft + feats + head + istft + crit, 'fused_bound': 2 * 4 * T,
            'parts': {'stft_2ch': stft, 'features': feats, 'head': head, 'istft_dbnorm': istft, 'criterion': crit}}


def main():
    wd = os.environ.get('SE_BENCH_WATCHDOG')          # seconds: every thread's Python stack on stderr if the run is still going then (hang diagnosis)
    if wd:
        import faulthandler
        import threading
        faulthandler.dump_traceback_later(float(wd), exit=False)

        def _native_threads():
            # what the NATIVE threads (gloo / RCCL workers, HIP runtime) are doing when the Python stacks say "everybody waits": name, scheduler
            # state and kernel wait channel of every thread of this process (round 3's four-rank gloo hang had only the Python side on record)
            lines = []
            for tid in sorted(os.listdir('/proc/self/task'), key=int):
                rec = []
                for f in ('comm', 'wchan'):
                    try:
                        rec.append(open(f'/proc/self/task/{tid}/{f}').read().strip() or '-')
                    except OSError:
                        rec.append('?')
                try:
                    st = [ln.split()[1] for ln in open(f'/proc/self/task/{tid}/status') if ln.startswith('State:')][0]
                except (OSError, IndexError):
                    st = '?'
                lines.append(f'  tid {tid:>8s} {st} {rec[0]:<24s} wchan {rec[1]}')
            sys.stderr.write(f'[watchdog] rank {os.environ.get("RANK", "0")}: native threads\n' + '\n'.join(lines) + '\n')
            sys.stderr.flush()
        t = threading.Timer(float(wd) + 1.0, _native_threads)
        t.daemon = True
        t.start()
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=1)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--batch', type=int, default=None, help='utterances per GPU per step (default: 32 = configs[1]; head workload: 256)')
    ap.add_argument('--layers', type=int, default=6, help='encoder depth (6 = config/pretrain_sample.yaml; 3 = "base")')
    ap.add_argument('--workload', choices=('enhance', 'finetune', 'lstm', 'head'), default='enhance',
                    help="enhance = configs[1] (the headline metric); head = configs[3] / configs[0] (vcb.yaml / pseudo_noise.yaml inference: "
                         "STFT -> LinearResidual mask -> iSTFT on (B, 2, T) noisy/clean batches, fp32, HBM-bound); finetune = configs[2]'s Mockingjay "
                         'training step (fwd + L1 + bwd + gradient all-reduce + clip + BertAdam); lstm = the same step for the 3 x BiLSTM-256 head of '
                         'pseudo_noise.yaml:50-53 on raw features (run_active.sh); all but enhance are side measurements')
    ap.add_argument('--head-feat', choices=tuple(HEAD_FEATS), default='mel120', help='head workload: the mask head\'s input features')
    ap.add_argument('--streams', type=int, default=1, help='process the batch as this many sub-batches on separate HIP streams (enhance workload)')
    ap.add_argument('--graph', action='store_true', help='replay the pass as one hipGraph launch (serving-size batches are launch-bound)')
    ap.add_argument('--full', action='store_true', help='after the timed steps also run the side legs and report them as extra keys of the line: the roofline '
                                                        'leg, the host-fed rate, the parity-mode / batch-12 rates, the CPU baseline (each has a --no-... switch)')
    ap.add_argument('--dump-outputs', metavar='DIR', default=None, help='write what the last timed step returned (rank 0) as DIR/<name>.npy, float32, '
                                                                        'at most 64 MB in all (a fixed seeded sample of a larger array)')
    ap.add_argument('--no-cpu-baseline', action='store_true')
    ap.add_argument('--no-roofline', action='store_true')
    ap.add_argument('--no-host-fed', action='store_true', help='skip the PCIe-inclusive side measurement')
    ap.add_argument('--no-extras', action='store_true', help='skip the extra keys of the default line (fp32 parity-mode rate, head batch-12 rate)')
    ap.add_argument('--backend', default='nccl', help="torch.distributed backend of the ranks ('nccl' = RCCL over xGMI)")
    ap.add_argument('--one-device', action='store_true', help='rehearsal: every rank uses cuda:0 (several ranks on a one-GPU box, e.g. --gpus 2 --backend gloo)')
    ap.add_argument('--launch-check', action='store_true', help='rank plumbing only (no kernels): used by the CPU test of the launcher')
    ap.add_argument('--stub-step', action='store_true', help='CPU rehearsal of the whole control flow: the step is a torch stub with the same collective '
                                                             'sequence (tests/test_dist_gloo.py); prints a line marked "stub"')
    args = ap.parse_args()
    if args.batch is None:
        args.batch = 256 if args.workload == 'head' else (4 if args.stub_step else 32)

    if args.gpus > 1 and 'RANK' not in os.environ:
        launch_ranks(args.gpus, sys.argv[1:])            # never returns; nothing above touched the GPU
    if args.launch_check:
        return launch_check(args)

    # RCCL prints a version banner on stdout at communicator creation; the contract is ONE JSON line on stdout, so
    # everything before the final print goes to stderr at the file-descriptor level.
    sys.stdout.flush()
    saved_stdout_fd = os.dup(1)
    os.dup2(2, 1)

    # ---------------- phase A: every rank, identical sequence of collectives ----------------
    ranks = Ranks(args)
    rank, world, dev = ranks.rank, ranks.world, ranks.dev
    w = build_stub_workload(args, ranks) if args.stub_step else build_workload(args, ranks)
    step, lib, wavs, lengths, max_len = w['step'], w['lib'], w['wavs'], w['lengths'], w['max_len']

    for _ in range(args.warmup):
        step(wavs, lengths, max_len)
    ranks.sync()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        wav_pred, loss, aux = step(wavs, lengths, max_len)
    ranks.local_sync()
    elapsed = time.perf_counter() - t0
    if ranks.distributed:
        ranks.dist.barrier()
    elapsed = ranks.max_over_ranks(elapsed)
    assert torch.isfinite(wav_pred).all() and torch.isfinite(loss)
    # what a caller of the timed path receives: the enhanced waveforms, the loss and the predicted spectrum (the training steps return the loss alone)
    dumped = snapshot_outputs((('wav_pred', None if w['collective'] else wav_pred), ('loss', loss), ('predicted', aux))) if args.dump_outputs else None

    do_roofline = args.full and not args.no_roofline and lib is not None
    if args.full and not args.no_roofline:
        # roofline leg: the same K steps with HIP events recorded (in-library, on the launch stream) around every kernel of the dominant
        # families.  EVERY rank runs it (the training steps all-reduce; and no rank-conditional code may sit between two collectives).
        if lib is not None:
            lib.se_prof_reset()
            lib.se_prof_enable(1)
        for _ in range(args.steps):
            step(wavs, lengths, max_len)
        ranks.local_sync()
        if lib is not None:
            lib.se_prof_enable(0)
    world_observed, was_distributed = ranks.world_observed, ranks.distributed
    ranks.teardown()                                         # last collective; from here on no rank can wait for another

    # ---------------- phase B: rank 0 only, collective-free by construction (the process group no longer exists) ----------------
    if rank != 0:
        return
    import torch.distributed as _d
    assert not (_d.is_available() and _d.is_initialized()), 'side legs must not run inside a process group'

    total_utts = args.batch * world * args.steps
    metric = {'enhance': 'enhanced 10s utts/sec', 'head': 'enhanced 10s utts/sec', 'finetune': 'fine-tuned 10s utts/sec (Mockingjay training step)',
              'lstm': 'trained 10s utts/sec (LSTM head training step)'}[args.workload]
    out = {
        'metric': metric, 'value': total_utts / elapsed, 'unit': 'utt/s', 'n_gpus': world_observed,
        'steps': args.steps, 'warmup': args.warmup, 'ms_per_step': 1000.0 * elapsed / args.steps,
        'higher_is_better': True, 'scaling': 'weak', 'vs_baseline': None, 'dtype': w['dtype'], 'data': 'synthetic',
        'config': {'workload': 'configs[1]: TERA/Mockingjay upstream (6x768x12x3072, pretrain_sample.yaml) + '
                               'TransformerSpecPredictionHead, evaluate()-style pass, 10 s @ 16 kHz',
                   'batch_per_gpu': args.batch, 'global_batch': args.batch * world, 'layers': args.layers,
                   'frames': 1001, 'parallelism': f'dp{world} (utterance-sharded inference, no data-path collective)',
                   'weights': 'seeded random, real sizes',
                   'ranks': f'{world_observed} ranks counted by all-reduce over {args.backend}' if was_distributed else 'single process, no process group'},
    }
    if args.stub_step:
        out['stub'] = 'control-flow rehearsal on CPU (torch stub step, same collective sequence); not a measurement'
    if args.graph and args.workload in ('enhance', 'head'):
        out['config']['launch'] = 'one hipGraph replay per step'
    if args.streams > 1 and args.workload == 'enhance':
        out['config']['streams'] = f'{args.streams} sub-batches of the batch in flight on separate HIP streams'
    if args.workload == 'lstm':
        out['config']['workload'] = ('config 5 style: 3 x BiLSTM-256 + Linear(512->201) head (pseudo_noise.yaml:50-53, 4.0 M params) on mel/log/delta-2 '
                                     'features: STFT/features, forward, masked log-L1, backward (BPTT), gradient all-reduce, clip 1.0, BertAdam')
        out['config']['parallelism'] = f'dp{world} (replicated parameters, one gradient all-reduce per step)'
    if args.workload == 'finetune':
        out['config']['workload'] = ('configs[2]: Mockingjay fine-tune step (6x768x12x3072 encoder + spec head, 43 M params): STFT/features, '
                                     'forward (train mode, dropout 0.1), masked log-L1, backward, per-layer bucketed gradient all-reduce, clip 1.0, BertAdam')
        out['config']['parallelism'] = f'dp{world} (replicated parameters, bucketed gradient all-reduce overlapped with the backward)'
    if args.workload == 'head':
        del out['config']['layers'], out['config']['weights']
        out['config']['workload'] = ('configs[3] / configs[0]: vcb.yaml / pseudo_noise.yaml inference-only enhancement, evaluate()-style pass on (B, 2, T) '
                                     'noisy/clean batches (NoisyCleanDataset): STFT of both channels -> ' +
                                     ('mel/log/delta-2 features (120) -> ' if args.head_feat == 'mel120' else 'linear power features (201, vcb.yaml:10-14) -> ') +
                                     'LinearResidual(cmvn, sigmoid) mask (.) noisy power -> iSTFT (noisy phase) -> level normalisation to the clean wav; '
                                     'SISDR criterion; exact fp32 throughout')
        if not args.stub_step:
            hb = head_pass_bytes(args.head_feat)
            per_s = out['value']
            out['pass_hbm'] = {'algorithmic_bytes_per_utt_sum_of_kernels': hb['sum_of_kernels'], 'parts': hb['parts'],
                               'achieved_GBs_sum_of_kernels': per_s * hb['sum_of_kernels'] / 1e9,
                               'frac_sum_of_kernels': per_s * hb['sum_of_kernels'] / 1e9 / HBM_PEAK_GBS,
                               'fused_bound_bytes_per_utt': hb['fused_bound'],
                               'achieved_GBs_vs_fused_bound': per_s * hb['fused_bound'] / 1e9,
                               'frac_vs_fused_bound': per_s * hb['fused_bound'] / 1e9 / HBM_PEAK_GBS,
                               'note': 'whole-pass view (SURVEY 8d): utterances/s x algorithmic bytes per utterance / 8 TB/s; `roofline` is the dominant kernel'}

    if do_roofline:
        roofline_report(args, lib, out)

    if dumped is not None:
        dump_outputs(args.dump_outputs, dumped)

    if args.full and not args.stub_step:
        if args.workload in ('enhance', 'head') and not args.graph and not args.no_host_fed:
            out['host_fed'] = host_fed_leg(args, w, dev)
        if not args.no_extras:
            extras_leg(args, w, dev, out)
        if world == 1 and not args.no_cpu_baseline and args.workload in ('enhance', 'head'):
            try:
                if args.workload == 'enhance':
                    out['cpu_baseline'] = cpu_baseline(batch=4, layers=args.layers, seconds_budget=28.0)
                else:
                    out['cpu_baseline'] = cpu_baseline_head(batch=16, head_feat=args.head_feat, seconds_budget=20.0)
            except Exception as e:      # the baseline is a reported extra; never lose the GPU line
                out['cpu_baseline'] = {'value': None, 'unit': 'utt/s', 'cores': os.cpu_count(), 'kind': 'port', 'sample': f'failed: {e}'}

    sys.stdout.flush()
    os.dup2(saved_stdout_fd, 1)
    os.close(saved_stdout_fd)
    print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
