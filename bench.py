#!/usr/bin/env python3
"""Headline benchmark: CLIP-Event contrastive TRAIN STEP on MI355X (BASELINE.json configs[1]).

One step = forward (ViT-B/32 image tower + 77-token text tower) + global-batch InfoNCE +
backward + clip_grad_norm_(.,1) + Adam, on synthetic 224px images / 77-token captions with
random-init weights, per-GPU batch 256, bf16 GEMM operands (fp32 accumulate / residual / master).

    python bench.py --gpus 1 --steps 10 --warmup 3
    python bench.py --gpus N ...          (no WORLD_SIZE in the environment: starts the N ranks itself, clip_event_amd/launch.py)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W

Prints ONE JSON line on rank 0 (contract in the task statement).  A plain run sets up, warms up, times
--steps steps and reports them; --full adds the measurements that need runs of their own or other hardware:
`roofline` (dominant kernel class, algorithmic FLOPs / HIP-event time measured in an instrumented pass of the
same step), `cpu_baseline` (the CPU oracle timed on the host cores, N=1 only), `config.dense_text` (the same step
with dense 77-row captions) and `power_sample` (board power / shader clock over the timed steps).
--dump-outputs DIR writes what the last timed step returned (its losses and a fixed sample of the updated parameters)
as DIR/<name>.npy.
"""
import argparse
import ctypes
import json
import os
import sys
import time

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

# per geometry: default per-GPU batch, nominal fwd+bwd FLOP per pair at K = 1 (BASELINE.md section 3 / SURVEY 8(d): ViT-B/32
# 44.10 G without the never-needed patch-conv dgrad; ViT-L/14@336 1185.7 G), the text tower's share of it per caption
# (ViT-B/32: 3 * 2 * 2.9798 GMAC; ViT-L/14: (1345.3 - 1185.7) / 4), name for the workload string
ARCH = {
    "vit_b32": (256, 44.10e9, 3 * 2 * 2.9798e9, "ViT-B/32 224px"),
    "vit_b16": (128, 3 * 2 * (17.58e9 + 2.9798e9), 3 * 2 * 2.9798e9, "ViT-B/16 224px"),
    "vit_l14_336": (32, 1185.7e9, (1345.3e9 - 1185.7e9) / 4, "ViT-L/14 336px"),
}
PEAK_BF16 = 2.5e15             # dense bf16 MFMA, MI355X_MICROARCH.md
PEAK_HBM = 8.0e12


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=None, help="per-GPU image batch (default: 256 for ViT-B/32, 32 for ViT-L/14@336)")
    ap.add_argument("--arch", default="vit_b32", choices=sorted(ARCH),
                    help="geometry: vit_b32 = the headline metric (BASELINE configs 1-4); vit_l14_336 = BASELINE config 5")
    ap.add_argument("--fp8", type=int, nargs="?", const=3, default=0,
                    help="BASELINE config 5's fp8 MFMA weight path: bit 0 forward GEMMs, bit 1 input-gradient GEMMs (bare --fp8 = 3)")
    ap.add_argument("--full", action="store_true",
                    help="also run the extra measurements after the timed steps: CPU oracle baseline, dense-text comparison, "
                         "instrumented roofline pass; and sample board power during them (a plain run only times the step)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step computed (its losses and a fixed seeded sample of the updated "
                         "parameters) as DIR/<name>.npy")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU oracle baseline")
    ap.add_argument("--no-roofline", action="store_true", help="with --full: skip the instrumented roofline pass")
    ap.add_argument("--descriptions", type=int, default=1,
                    help="descriptions per image K (1 positive + K-1 hard negatives, BASELINE config 3 uses 5); the "
                         "headline metric is K = 1")
    ap.add_argument("--dense-text", action="store_true",
                    help="run the text tower on all 77 positions of every caption (default: live tokens SOT..EOT only; "
                         "a --full run also reports this dense variant as config.dense_text)")
    ap.add_argument("--no-dense-compare", action="store_true", help="with --full: skip the dense-text comparison run")
    ap.add_argument("--reuse-captions", action="store_true",
                    help="hand the model the SAME caption tensor every step (its live-token layout is then cached; the "
                         "default gives every step a new tensor, so the per-batch length read-back of real training is "
                         "inside the timed region)")
    ap.add_argument("--device-lengths", action="store_true",
                    help="do not hand the captions' host-side lengths to the step: the text tower then reads the EOT "
                         "positions back from the device once per new caption tensor (a synchronous 1 KB copy)")
    ap.add_argument("--alignment", action="store_true",
                    help="BASELINE config 4: add sim_entity + the IPOT alignment loss (object crops / entity mentions "
                         "as SURVEY 8(d) c4: 1+U[0,6] objects, U[1,10] entities per image)")
    ap.add_argument("--train-arg", default=None, choices=["desc", "desc_type", "desc_type_text"],
                    help="BASELINE config 4: add the region / argument branch (U[1,4] roles per image, 25%% None boxes)")
    ap.add_argument("--cu-hog", type=int, default=0,
                    help="diagnostic (DESIGN 5): hold this many CUs busy-idle on a third stream for the length of every step "
                         "(ce_cu_hog), as an RCCL ring's channel kernels would during the gradient all-reduce")
    ap.add_argument("--single-stream", action="store_true",
                    help="run both towers on one stream (the default overlaps them on two)")
    return ap.parse_args()


def log(msg):
    print(f"[bench] {msg}", file=sys.stderr, flush=True)


def host_cores() -> int:
    """Threads this process may really use: affinity mask, capped by the cgroup CPU quota and by 16
    (the GPU box's CPU share per GPU); oversubscribing the host makes the CPU oracle crawl."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            n = min(n, max(1, int(int(quota) / int(period))))
    except Exception:
        pass
    return max(1, min(n, 16))


def cpu_model() -> str:
    try:
        for line in open("/proc/cpuinfo"):
            if line.lower().startswith("model name"):
                return line.split(":", 1)[1].strip()
    except Exception:
        pass
    import platform
    return platform.processor() or platform.machine()


def cpu_baseline():
    """The CPU oracle (plain PyTorch fp32 restatement of the reference) on this host's cores, SURVEY 8(d): config c1
    exactly (ViT-B/32, B = 8, caption-only InfoNCE, full step with clip + Adam) plus B = 32 for a fairer per-pair figure;
    1 warm-up step + >= 5 timed steps (3 at B = 32 if they are slow), median reported, bounded to ~30 s of CPU work."""
    import statistics
    from oracle import clip_oracle as O
    from clip_event_amd import synthetic as S
    cores = host_cores()
    torch.set_num_threads(cores)
    log(f"cpu baseline on {cores} threads ({cpu_model()})")

    def leg(B, min_steps, max_steps, budget):
        p = O.init_params(O.VIT_B32, 0)
        img = S.synthetic_images(B, 224, seed=999)
        txt = S.synthetic_tokens(B, 77, 49408, seed=999)
        y = torch.arange(B)
        state = {}
        t0 = time.time()
        p, _, _ = O.train_step(p, O.VIT_B32, state, img, txt, y, y, y)     # warm-up
        warm = time.time() - t0
        times, t_start = [], time.time()
        while len(times) < min_steps or (time.time() - t_start < budget and len(times) < max_steps):
            t1 = time.time()
            p, _, _ = O.train_step(p, O.VIT_B32, state, img, txt, y, y, y)
            times.append(time.time() - t1)
            if warm > 30 and len(times) >= 1:
                break
        med = statistics.median(times)
        log(f"cpu baseline B={B}: warm-up {warm:.1f}s, {len(times)} timed steps, median {med:.2f}s/step")
        return {"value": round(B / med, 3), "steps": len(times), "median_s_per_step": round(med, 3)}

    b8 = leg(8, 5, 8, 10.0)
    b32 = leg(32, 3, 5, 14.0)
    return {"value": b8["value"], "unit": "pairs/s", "cores": torch.get_num_threads(), "kind": "port", "cpu": cpu_model(),
            "sample": f"median of {b8['steps']} full train steps (after 1 warm-up) of ViT-B/32 at batch 8 (BASELINE config 1), fp32, "
                      f"CPU oracle; batch 32: median of {b32['steps']} steps",
            "batch_32": {"value": b32["value"], "unit": "pairs/s", "steps": b32["steps"]}}


def pmc_traffic(kernel_class):
    """HBM bytes per launch of the dominant kernel from the committed rocprofv3 PMC passes (FETCH_SIZE x2-corrected
    + WRITE_SIZE, tools/pmc_traffic.py; PMC needs its own runs, so bench.py cannot collect it live)."""
    import glob
    import re

    def version_key(path):          # r02_..._v10.json sorts after r02_..._v9.json, and r02 after r01
        nums = [int(x) for x in re.findall(r"\d+", os.path.basename(path))]
        return (nums, os.path.getmtime(path))

    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_pmc_hbm_traffic*.json")), key=version_key)
    if not files:
        return None, None
    # class name -> rocprofv3 kernel row: "gemm_nt256_kernel<0,*,2> BF16" matches "gemm_nt256_kernel<0, 5, 2>";
    # "gemm_tn" matches "gemm_tn3_kernel<48, 3>" (rows are sorted by total time: first match = the one that dominates)
    head = kernel_class.split(" ")[0]
    rx = "".join("\\d+" if ch == "*" else (",\\s*" if ch == "," else re.escape(ch)) for ch in head)
    pat = re.compile("^" + rx + ("$" if "<" in head else ""))
    try:
        for row in json.load(open(files[-1])):
            if pat.match(row["kernel"]):
                return (row["fetch_corrected_x2_MB"] + row["WRITE_SIZE_MB_per_launch"]) * 1e6, os.path.basename(files[-1])
    except Exception:
        pass
    return None, None


def mfma_util():
    """MFMA utilisation per kernel class from the committed rocprofv3 PMC pass (SQ_VALU_MFMA_BUSY_CYCLES /
    SQ_BUSY_CU_CYCLES, tools/pmc_mfma.py); PMC needs its own run, so bench.py reads the summary."""
    import glob
    import re
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_pmc_mfma_util*.json")),
                   key=lambda f: ([int(x) for x in re.findall(r"\d+", os.path.basename(f))], os.path.getmtime(f)))
    if not files:
        return None
    try:
        return {"source": os.path.basename(files[-1]), "kernels": json.load(open(files[-1]))[:8]}
    except Exception:
        return None


class PowerSampler:
    """Board power and shader clock from the amdgpu hwmon files of this rank's GPU, sampled in a thread while the timed steps
    run: stored beside every bench line so that box-to-box spread (clock / power state of the part) can be told from a
    regression.  Reading sysfs touches neither HIP nor the GPU's queues; silently empty where the files
    are not there."""

    def __init__(self, index: int = 0, period: float = 0.02):
        import glob
        self.files = {}
        gpus = []
        try:        # the hwmon directory of THIS device, by PCI address (a box shows every GPU of its host in sysfs)
            pr = torch.cuda.get_device_properties(index)
            addr = "%04x:%02x:%02x.0" % (pr.pci_domain_id, pr.pci_bus_id, pr.pci_device_id)
            gpus = sorted(glob.glob(f"/sys/bus/pci/devices/{addr}/hwmon/hwmon*"))
            index = 0
        except Exception:
            pass
        if not gpus:
            cards = sorted(glob.glob("/sys/class/drm/card[0-9]*/device/hwmon/hwmon*"))
            gpus = [c for c in cards if glob.glob(os.path.join(c, "power1_*"))]
        if gpus:
            base = gpus[min(index, len(gpus) - 1)]
            for key, names in (("power_w", ("power1_average", "power1_input")), ("sclk_mhz", ("freq1_input",)),
                               ("power_cap_w", ("power1_cap",)), ("temp_c", ("temp1_input",))):
                for n in names:
                    if os.path.exists(os.path.join(base, n)):
                        self.files[key] = os.path.join(base, n)
                        break
        self.scale = {"power_w": 1e-6, "power_cap_w": 1e-6, "sclk_mhz": 1e-6, "temp_c": 1e-3}
        self.period, self.samples, self._stop, self._th = period, {k: [] for k in self.files}, False, None

    def _run(self):
        while not self._stop:
            for k, f in self.files.items():
                try:
                    self.samples[k].append(float(open(f).read().strip()) * self.scale[k])
                except Exception:
                    pass
            time.sleep(self.period)

    def start(self):
        if self.files:
            import threading
            self._stop = False
            self._th = threading.Thread(target=self._run, daemon=True)
            self._th.start()

    def stop(self):
        self._stop = True
        if self._th is not None:
            self._th.join(timeout=1.0)
        out = {}
        for k, v in self.samples.items():
            if v:
                out[k] = {"mean": round(sum(v) / len(v), 1), "min": round(min(v), 1), "max": round(max(v), 1), "n": len(v)}
        return out or None


class OutputDump:
    """``--dump-outputs DIR``: what a caller of ``train_step`` holds after the last timed step, as .npy files, for comparing
    two builds output for output.  ``loss_<name>.npy``: the loss dict the last step returned (float64 scalars).
    ``params_sample.npy``: the updated parameters at a fixed, seeded set of 2^21 positions of their concatenation in name
    order (ViT-B/32: ~150 M values; float32, 8 MB), gathered per parameter without a copy of the model.

    Both depend on the gradients: over the default 3 + 10 steps the loss falls from 11.16 to 10.87 and the parameters move
    by ~4.5e-4 (relative L2), against run-to-run spreads of ~2e-5 and ~5e-6.  The gradients and the parameter update
    themselves are not written: from one state the step's gradients agree to ~2e-8 between runs, but each step re-draws
    the bf16 rounding of a state that differs in the last bits, so after a few steps they differ by ~1.5 % from run to
    run, the size of their own bf16 rounding error, and could not be compared output for output."""

    SAMPLES = 1 << 21
    SEED = 20240601

    def __init__(self, model, out_dir):
        import numpy as np
        self.model, self.dir = model, out_dir
        named = sorted(model.named_parameters(), key=lambda t: t[0])
        starts = np.concatenate([[0], np.cumsum([p.numel() for _, p in named])]).astype(np.int64)
        idx = np.sort(np.random.default_rng(self.SEED).choice(int(starts[-1]), size=min(self.SAMPLES, int(starts[-1])),
                                                              replace=False))
        dev = next(model.parameters()).device
        # per parameter, the sampled positions inside it
        cut = np.searchsorted(idx, starts)
        self.picks = [(n, torch.from_numpy(idx[cut[i]:cut[i + 1]] - starts[i]).to(dev))
                      for i, (n, _) in enumerate(named) if cut[i + 1] > cut[i]]

    def write(self, loss_dict):
        import numpy as np
        os.makedirs(self.dir, exist_ok=True)
        params = dict(self.model.named_parameters())
        out = {"loss_" + k.removeprefix("loss_"): v.detach().double().reshape(()) for k, v in loss_dict.items()}
        out["params_sample"] = torch.cat([params[n].detach().reshape(-1)[local].float() for n, local in self.picks])
        for name, t in out.items():
            np.save(os.path.join(self.dir, name + ".npy"), t.cpu().numpy())
        log(f"outputs of the last timed step -> {self.dir}: {', '.join(sorted(out))}")


def ms_per_step_tmp(dt, steps):
    return dt / steps * 1e3


def main():
    args = parse()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # one command starts the ranks (the reference's launch contract: train.sh:2, utils.py:541-616): N fresh child
        # interpreters, one per GPU, BEFORE this process makes any device call; rank 0's JSON line is relayed.
        from clip_event_amd.launch import spawn_ranks, visible_gpus
        visible = visible_gpus()                     # visibility variables / KFD sysfs: no HIP call in the parent
        if visible and visible < args.gpus and not os.environ.get("CE_ALL_RANKS_ON_GPU0"):
            log(f"--gpus {args.gpus} but only {visible} GPU(s) visible (CE_ALL_RANKS_ON_GPU0=1 rehearses the ranks on one GPU over gloo)")
            sys.exit(2)
        sys.exit(spawn_ranks(args.gpus, [sys.executable, os.path.abspath(__file__), *sys.argv[1:]]))
    W = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if W > 1 and args.gpus != W:
        log(f"--gpus {args.gpus} but the launcher started WORLD_SIZE={W} ranks: reporting the live process group")
    if os.environ.get("CE_ALL_RANKS_ON_GPU0"):      # rehearsal of the N>1 path on a one-GPU box: RCCL refuses two
        local_rank = 0                              # ranks on one device, so the rehearsal runs the collectives on gloo
        os.environ.setdefault("CE_DIST_BACKEND", "gloo")
    force = os.environ.get("CE_FORCE_COLLECTIVES", "0") == "1"    # one rank, but through every RCCL call
    real_stdout = None
    if W > 1 or force:
        # RCCL prints a version banner on STDOUT when its first communicator comes up: keep the contract (ONE JSON line on
        # stdout) by pointing fd 1 at stderr for the run and writing the result line to the saved descriptor
        sys.stdout.flush()
        real_stdout = os.dup(1)
        os.dup2(2, 1)
    if W > 1 or force:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if "MASTER_PORT" not in os.environ:                          # single-rank rehearsal: any free port
            import socket
            with socket.socket() as sk:
                sk.bind(("127.0.0.1", 0))
                os.environ["MASTER_PORT"] = str(sk.getsockname()[1])
        os.environ.setdefault("RANK", "0")
        os.environ.setdefault("WORLD_SIZE", "1")
        torch.cuda.set_device(local_rank)
        backend = os.environ.get("CE_DIST_BACKEND", "nccl")          # "nccl" == RCCL on ROCm; gloo only to rehearse
        if backend == "nccl":                                        # several ranks on a one-GPU box
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
        else:
            dist.init_process_group(backend)
    dev = torch.device("cuda", local_rank)
    torch.cuda.set_device(dev)
    if dist.is_initialized():                                        # the live process group, not the environment
        W, rank = dist.get_world_size(), dist.get_rank()
    rccl_ranks = W if (dist.is_initialized() and dist.get_backend() == "nccl") else 0

    from clip_event_amd import synthetic as S
    from clip_event_amd import distributed as D
    from clip_event_amd._lib import lib
    from clip_event_amd.engine import train_step
    from clip_event_amd.losses import CriterionContrastive
    from clip_event_amd.model import build_model
    from clip_event_amd.optim import FusedAdam

    B_default, FLOP_PER_PAIR, TEXT_FLOP_PER_PAIR, arch_name = ARCH[args.arch]
    B = args.batch or B_default
    model = S.synthetic_model(args.arch, seed=0).to(dev)         # same weights on every rank
    model.fp8 = int(args.fp8)
    R = model.visual.input_resolution
    model.tower_streams = not args.single_stream
    crit = CriterionContrastive("ce")
    opt = FusedAdam(model, lr=1e-6, weight_decay=0.0, max_norm=1.0)    # README.md:189-191 defaults
    sync = D.GradSync(model) if ((W > 1 or force) and os.environ.get("CE_NO_GRAD_SYNC", "0") != "1") else None
    img = S.synthetic_images(B, R, seed=999 + rank).to(dev)
    K = max(1, args.descriptions)
    txt_host = S.synthetic_tokens(B * K, 77, 49408, seed=999 + rank)
    txt = txt_host.to(dev)
    yi, yt, ip = D.global_labels(B, 1, K - 1, True, device=dev, rank_=rank)
    extra = {}
    if args.alignment:
        from clip_event_amd.losses import CriterionAlignment
        model.set_hyps(True, True, False)
        obj, obj_num, ent, ent_num = S.synthetic_entities(B, R, 77, 49408, seed=1999 + rank)
        from clip_event_amd.functional import tokens_to_device
        extra.update(criterion_ot=CriterionAlignment(), object_vec=obj.to(dev), entitytxt_vec=tokens_to_device(ent, dev),
                     object_num=obj_num.to(dev), entitytxt_num=ent_num.to(dev))     # (tokens_to_device: .to(dev) + host-side lengths)
        log(f"alignment: object_vec {tuple(obj.shape)}, entitytxt_vec {tuple(ent.shape)}")
    if args.train_arg:
        boxes = S.synthetic_bboxes(B, seed=2999 + rank)
        from clip_event_amd.functional import tokens_to_device
        extra.update(train_arg=args.train_arg, bboxs=boxes,
                     bbox_desc_vec=[tokens_to_device(t, dev) for t in S.synthetic_role_texts(boxes, seed=3999 + rank)],
                     bbox_label_vec=[tokens_to_device(t, dev) for t in S.synthetic_role_texts(boxes, seed=4999 + rank)])

    # what one step pushes through the towers: images / captions of the main batch plus, in config 4, the object crops and
    # entity mentions of sim_entity (engine.py:57-63; padding slots are encoded too, as in the reference) and the role
    # descriptions (+ labels) of the usable boxes of the region branch (model_clip.py:430-488)
    n_img, n_txt = B, B * K
    txt_live = int((txt_host.argmax(dim=-1) + 1).sum())
    if args.alignment:
        n_img += obj.shape[0] * obj.shape[1]
        n_txt += ent.shape[0] * ent.shape[1]
        txt_live += int((ent.reshape(-1, ent.shape[-1]).argmax(dim=-1) + 1).sum())
    if args.train_arg:
        reps = 2 if args.train_arg.startswith("desc_type") else 1
        for bx, rows_ in zip(boxes, extra["bbox_desc_vec"]):
            if not bx or bx[-1] is None:                      # model_clip.py:450-455: the image contributes nothing
                continue
            use = [i for i, b_ in enumerate(bx) if b_ is not None]
            n_txt += reps * len(use)
            txt_live += reps * int((rows_[use].argmax(dim=-1) + 1).sum())

    if args.dense_text:
        model.pack_text = False

    # the data loader's side of the contract: every step gets a NEW caption tensor in HBM (fresh storage, as a real batch
    # would be) together with the captions' lengths, which the tokenizer knows on the host (clip.tokenize / attach_lengths);
    # --device-lengths withholds them, so the text tower reads the EOT positions back from the device each step
    from clip_event_amd.functional import attach_lengths, host_lengths
    txt_lens = None if args.device_lengths else host_lengths(txt_host)

    hog = {"stream": torch.cuda.Stream(device=dev) if args.cu_hog else None, "us": 0.0}

    def step():
        t = txt if args.reuse_captions else txt.clone()
        if txt_lens is not None:
            attach_lengths(t, txt_lens)
        if args.cu_hog and hog["us"] > 0:
            # the hog starts with the step (its stream waits for the previous step's end) and lasts one un-hogged step time
            hog["stream"].wait_stream(torch.cuda.current_stream())
            lib().ce_cu_hog(ctypes.c_int(args.cu_hog), ctypes.c_float(hog["us"]), ctypes.c_void_p(hog["stream"].cuda_stream))
            out = train_step(model, crit, opt, img, t, yi, yt, ip, grad_sync=sync, **extra)
            torch.cuda.current_stream().wait_stream(hog["stream"])
            return out
        return train_step(model, crit, opt, img, t, yi, yt, ip, grad_sync=sync, **extra)

    def timed(nsteps):
        if W > 1:
            dist.barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(nsteps):
            out = step()
        torch.cuda.synchronize()
        if W > 1:
            dist.barrier()
        dt = time.perf_counter() - t0
        if W > 1:
            t = torch.tensor([dt], device=dev, dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            dt = float(t)
        return dt, out

    dump = OutputDump(model, args.dump_outputs) if (args.dump_outputs and rank == 0) else None
    for _ in range(args.warmup):
        ld = step()
    if args.cu_hog:          # calibrate the hog's duration on the un-hogged step, then warm up again with it
        dt0, _ = timed(max(5, args.steps // 2))
        hog["us"] = dt0 / max(5, args.steps // 2) * 1e6
        log(f"cu hog: {args.cu_hog} CUs for {hog['us']:.0f} us per step (un-hogged step {hog['us'] / 1e3:.2f} ms)")
        for _ in range(2):
            step()
    sampler = PowerSampler(local_rank) if args.full else None
    if sampler is not None:
        sampler.start()
    dt, ld = timed(args.steps)
    power = sampler.stop() if sampler is not None else None
    if dump is not None:
        dump.write(ld)
    loss = float(sum(v.detach() for v in ld.values()))
    hog_mhz = None
    if args.cu_hog:
        lib().ce_cu_hog_clock_mhz.restype = ctypes.c_double
        hog_mhz = round(float(lib().ce_cu_hog_clock_mhz()), 1)
        log(f"cu hog: shader clock seen by the hog during the last step {hog_mhz} MHz")
    log(f"timed region: {ms_per_step_tmp(dt, args.steps):.2f} ms/step")
    ms_per_step = dt / args.steps * 1e3
    pairs_per_s = B * W * args.steps / dt
    # text rows the tower actually ran on (live tokens SOT..EOT) vs the dense [B, 77] layout
    live_frac = 1.0 if args.dense_text else txt_live / float(n_txt * 77)
    dense = None
    if args.full and not args.dense_text and not args.no_dense_compare and not extra and args.arch == "vit_b32":      # the same step with every caption padded out to 77 rows, for comparison
        model.pack_text = False
        nd = max(5, args.steps // 2)
        for _ in range(2):
            step()
        dtd, _ = timed(nd)
        model.pack_text = True
        dense = {"ms_per_step": round(dtd / nd * 1e3, 3), "value": round(B * W * nd / dtd, 2), "steps": nd}
        log(f"dense-text variant: {dense['ms_per_step']:.2f} ms/step")
        step()

    roof = None
    profile = args.full and not args.no_roofline
    if profile:     # every rank runs the instrumented steps (they contain collectives); rank 0 reports
        # instrumented pass: HIP events on the launch stream around every launch, summed per kernel class
        cl = lib()
        cl.ce_profile_class_name.restype = ctypes.c_char_p
        # kernels are timed in isolation: both towers on ONE stream for this pass (in the timed region they
        # overlap on two streams, which would stretch every per-kernel duration)
        model.tower_streams = False
        for _ in range(2):
            step()
        torch.cuda.synchronize()
        cl.ce_profile_enable(1)
        n_prof = 2
        for _ in range(n_prof):
            step()
        torch.cuda.synchronize()
        ncls = int(cl.ce_profile_num_classes())
        buf = (ctypes.c_double * (ncls * 4))()
        cl.ce_profile_collect(buf, ncls)
        cl.ce_profile_enable(0)
        model.tower_streams = not args.single_stream
        log("instrumented pass collected")
        rows = []
        for c in range(ncls if rank == 0 else 0):
            cnt, ms, fl, by = buf[c * 4:(c + 1) * 4]
            if cnt > 0:
                rows.append({"kernel": cl.ce_profile_class_name(c).decode(), "launches_per_step": cnt / n_prof,
                             "ms_per_step": ms / n_prof, "avg_us": ms / cnt * 1e3,
                             "tflops": fl / (ms * 1e-3) / 1e12 if ms > 0 else 0.0,
                             "gbps": by / (ms * 1e-3) / 1e9 if ms > 0 else 0.0})
        rows.sort(key=lambda r: -r["ms_per_step"])
        issued_flops = sum(r["tflops"] * 1e12 * r["ms_per_step"] * 1e-3 for r in rows)
    if rank == 0 and profile and rows:
        top = rows[0]
        mfma = top["kernel"].startswith("gemm") or top["kernel"].startswith("attn")
        ach = top["tflops"] if mfma else top["gbps"]
        peak = PEAK_BF16 / 1e12 if mfma else PEAK_HBM / 1e9
        traffic, traffic_src = pmc_traffic(top["kernel"])
        roof = {"bound": "mfma" if mfma else "hbm", "kernel": top["kernel"], "achieved": round(ach, 2), "peak": peak,
                "unit": "TFLOP/s" if mfma else "GB/s", "frac": round(ach / peak, 4), "traffic": traffic,
                "traffic_unit": "HBM bytes per launch (PMC FETCH_SIZE x2 + WRITE_SIZE)", "traffic_source": traffic_src,
                "algorithmic_bytes_per_launch": round(top["gbps"] * 1e9 * top["avg_us"] * 1e-6),
                "avg_launch_us": round(top["avg_us"], 2), "launches_per_step": top["launches_per_step"],
                # step_frac = the FLOPs the kernels of one step ISSUE (sum over the instrumented pass's classes: packed text
                # rows, the pruned last block of each tower and the loss head as they really run) / the timed step / peak:
                # the hardware utilisation, and the figure to hold against the 40 % target.  The two figures after it price the
                # step by the analytic model instead: every image at the image tower's and every caption at the text tower's
                # share of SURVEY 8(d)'s FLOP per pair -- with the text share scaled by the live-row fraction ("model"), and
                # with all 77 positions ("nominal": comparable with dense-text implementations, overstates what ran).
                "step_frac": round(issued_flops / (ms_per_step * 1e-3) / PEAK_BF16, 4),
                "issued_tflop_per_step": round(issued_flops / 1e12, 4),
                "step_frac_model_live_text_rows": round(
                    (n_img * (FLOP_PER_PAIR - TEXT_FLOP_PER_PAIR) + n_txt * TEXT_FLOP_PER_PAIR * live_frac)
                    / (ms_per_step * 1e-3) / PEAK_BF16, 4),
                "step_frac_nominal": round(
                    (n_img * (FLOP_PER_PAIR - TEXT_FLOP_PER_PAIR) + n_txt * TEXT_FLOP_PER_PAIR) / (ms_per_step * 1e-3) / PEAK_BF16, 4),
                "nominal_gflop_per_pair": round(FLOP_PER_PAIR / 1e9, 2),
                "tower_rows_per_step": {"images": n_img, "captions": n_txt, "live_text_row_fraction": round(live_frac, 4)},
                "mfma_utilisation": mfma_util(),
                "classes": [{k: (round(v, 3) if isinstance(v, float) else v) for k, v in r.items()} for r in rows]}
    if W > 1:
        dist.barrier()

    cpu = None
    if rank == 0 and W == 1 and args.full and not args.no_cpu_baseline:
        cpu = cpu_baseline()

    if rank == 0:
        out = {
            "metric": "image-text pairs/sec/GPU, %s x 77-tok, global-batch contrastive" % arch_name,
            "value": round(pairs_per_s, 2), "unit": "pairs/s (whole job)", "per_gpu": round(pairs_per_s / W, 2),
            "n_gpus": W, "rccl_ranks": rccl_ranks, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(ms_per_step, 3),
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "fp8" if args.fp8 else "bf16", "data": "synthetic",
            "config": {"workload": "%s x 77-tok, %s, per-GPU batch %d, K=%d, %s, full train step "
                                   "(fwd+bwd+clip_grad_norm+Adam), random-init weights"
                                   % (arch_name, ("fp8 (e4m3) weight path, bits %d" % args.fp8) if args.fp8 else "bf16 operands", B, K,
                                      "InfoNCE only" if not extra else "InfoNCE" + (" + OT alignment" if args.alignment else "")
                                      + (" + region branch (%s)" % args.train_arg if args.train_arg else "")),
                       "global_batch": B * W, "parallelism": "dp%d" % W, "loss": round(loss, 4),
                       "captions": "SOT + U[8,75] random ids + EOT, zero-padded to 77 (SURVEY 8(d) c2)",
                       "text_rows": ("all 77 positions" if args.dense_text else
                                     "live tokens SOT..EOT only: %.1f%% of B*77 rows (identical results, see DESIGN.md)"
                                     % (100.0 * live_frac)),
                       "fresh_captions_every_step": not args.reuse_captions,
                       "alignment": bool(args.alignment), "train_arg": args.train_arg, "cu_hog": args.cu_hog, "cu_hog_shader_clock_mhz": hog_mhz,
                       "nt_pgrid": int(os.environ.get("CE_NT_PGRID", "256")), "full": bool(args.full),
                       "dense_text": dense},
            "roofline": roof, "cpu_baseline": cpu,
            "power_sample": power,      # board power / shader clock (hwmon) over the timed steps of rank 0
        }
        if real_stdout is not None:
            os.write(real_stdout, (json.dumps(out) + "\n").encode())
        else:
            print(json.dumps(out), flush=True)
    if W > 1 or force:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
