"""Driver benchmark contract: flagship decode throughput.

Measures BASELINE.json's metric — decode tokens/sec (+ p50 step latency) for
Llama-3-8B greedy decode, sharded over N MI355X workers as a micro-batched
pipeline over RCCL/xGMI (bloombee_amd/parallel/pipeline.py). Synthetic data,
random-init weights (no network in this environment), bf16.

Weak scaling: global_batch = batch_per_gpu * N (per-GPU work fixed as N grows).

  python bench.py --gpus N --steps K --warmup W
  (N>1 is launched by the driver via torch.distributed.run, one rank per GPU)

A plain run sets up, warms up, times the K steps and prints one JSON result
line. --dump-outputs DIR additionally writes what the last timed step
returned (DIR/<name>.npy; inputs and weights are seeded, so the same
arguments give the same arrays run to run). --full is reserved for
measurements beyond the headline figure; there are none today.
"""
from __future__ import annotations

import argparse
import json
import os
import time

import torch


def stage_max_pos(model: str) -> int:
    from bloombee_amd.models.base import resolve_config

    return resolve_config(model).max_position_embeddings


DUMP_MAX_BYTES = 64 << 20  # cap on everything --dump-outputs writes


def dump_outputs(out_dir: str, arrays: dict) -> None:
    """Write what the last timed step returned to its caller as
    <out_dir>/<name>.npy (float32; token ids < 2^24 are exact). An output
    past its share of DUMP_MAX_BYTES is cut to a fixed seeded sample of
    its flattened elements, so two builds dump the same positions."""
    import numpy as np

    os.makedirs(out_dir, exist_ok=True)
    budget = DUMP_MAX_BYTES // max(1, len(arrays)) // 4 - 64  # elements, less header
    for name, t in arrays.items():
        a = t.detach().to("cpu", torch.float32).numpy()
        if a.size > budget:
            idx = np.sort(np.random.default_rng(0).choice(
                a.size, size=budget, replace=False))
            a = a.reshape(-1)[idx]
        np.save(os.path.join(out_dir, f"{name}.npy"), a)


def run_swarm(args):
    """The REAL decentralized serving stack under the bench contract: one
    Server (DHT + rpc_inference handler + paged-KV backend) per rank/GPU,
    the client on rank 0, every activation hop on the RCCL/xGMI device
    plane (net/channels.py) — VERDICT r01 item 1's "bench mode that runs
    the real Server/session stack"."""
    import torch.distributed as dist
    import torch.nn.functional as F

    from bloombee_amd import ops
    from bloombee_amd.client.config import ClientConfig
    from bloombee_amd.client.routing import RemoteSequenceManager
    from bloombee_amd.client.session import InferenceSession
    from bloombee_amd.models.base import resolve_config
    from bloombee_amd.net.channels import channels
    from bloombee_amd.net.dht import Dht
    from bloombee_amd.parallel.pipeline import init_distributed, layer_range
    from bloombee_amd.server import Server

    device = init_distributed("cpu" if args.device == "cpu" else "auto")
    if args.device:
        device = args.device
    rank = dist.get_rank() if dist.is_initialized() else 0
    world = dist.get_world_size() if dist.is_initialized() else 1
    on_gpu = device.startswith("cuda")
    channels.enable(device)  # collective when dist is initialized

    cfg = resolve_config(args.model)
    global_batch = args.batch_per_gpu * world
    session_len = args.prompt + args.steps + args.warmup + 8
    kv_tokens = global_batch * ((session_len + 15) // 16 + 1) * 16 + 1024

    # micro-batch policy for the GPU swarm: decode kernels lose ~2x below 8
    # rows (bench_kernels), so slices are per-GPU-batch sized; single-stage
    # worlds never split
    os.environ.setdefault("BBAMD_MICRO_BATCH_SIZE", str(args.batch_per_gpu))
    os.environ.setdefault("BBAMD_MIN_BATCH_TO_SPLIT",
                          str(2 * args.batch_per_gpu))

    # loopback DHT bootstrap: rank 0 owns it and shares the endpoint
    if dist.is_initialized():
        boot_ep = [None]
        boot = None
        if rank == 0:
            boot = Dht()
            boot_ep = [boot.endpoint]
        dist.broadcast_object_list(boot_ep, src=0)
        boot_ep = boot_ep[0]
    else:
        boot = Dht()
        boot_ep = boot.endpoint

    start, end = layer_range(cfg.num_hidden_layers, rank, world)
    server = Server(args.model, initial_peers=[boot_ep],
                    block_indices=(start, end), device=device, seed=0,
                    kv_max_tokens=kv_tokens, update_period=10.0,
                    max_batch_size=max(2048, global_batch))
    server.run_in_background()

    def _wait_done(dht):
        while not dht.get("bench_done"):
            time.sleep(0.5)

    if rank != 0:
        # workers serve until the client posts the done flag (no dist
        # collectives during decode: the data plane owns the comm)
        local_dht = server.dht
        _wait_done(local_dht)
        server.shutdown()
        channels.disable()
        if dist.is_initialized():
            dist.destroy_process_group()
        return

    # ---- rank 0: the client -------------------------------------------
    ccfg = ClientConfig(initial_peers=[boot_ep], keep_history=False,
                        update_period=10.0)
    manager = RemoteSequenceManager(ccfg, args.model, cfg.num_hidden_layers)
    deadline = time.monotonic() + 120
    while True:
        try:
            manager.update()
            route = manager.make_sequence(0, cfg.num_hidden_layers)
            if len(route) == world:
                break
        except Exception:
            pass
        if time.monotonic() > deadline:
            raise RuntimeError("swarm did not converge to a full route")
        time.sleep(0.5)

    gen = torch.Generator().manual_seed(0)
    dt = cfg.dtype
    dev = torch.device(device)
    embed = (torch.randn(cfg.vocab_size, cfg.hidden_size, generator=gen)
             .mul_(0.02).to(dt).to(dev))
    norm_w = torch.ones(cfg.hidden_size, dtype=dt, device=dev)
    lm_head_w = embed if cfg.tie_word_embeddings else (
        torch.randn(cfg.vocab_size, cfg.hidden_size, generator=gen)
        .mul_(0.02).to(dt).to(dev))

    session = InferenceSession(manager, max_length=session_len, config=ccfg)
    prompt = torch.randint(0, cfg.vocab_size, (global_batch, args.prompt),
                           generator=gen)
    CH = 512
    out = None
    for c0 in range(0, args.prompt, CH):
        chunk = prompt[:, c0:c0 + CH].to(dev)
        out = session.step(F.embedding(chunk, embed))

    def _lm_head(hidden_last):
        y = ops.rms_norm(hidden_last, norm_w, cfg.rms_norm_eps)
        return F.linear(y, lm_head_w).float().argmax(-1)

    ids = _lm_head(out[:, -1])
    for _ in range(args.warmup):
        out = session.step(F.embedding(ids.view(-1, 1), embed))
        ids = _lm_head(out[:, -1])
    if on_gpu:
        torch.cuda.synchronize()
    t0 = time.monotonic()
    step_ms = []
    for _ in range(args.steps):
        s0 = time.monotonic()
        out = session.step(F.embedding(ids.view(-1, 1), embed))
        ids = _lm_head(out[:, -1])
        if on_gpu:
            torch.cuda.synchronize()
        step_ms.append((time.monotonic() - s0) * 1e3)
    if on_gpu:
        torch.cuda.synchronize()
    elapsed = time.monotonic() - t0

    if args.dump_outputs:
        dump_outputs(args.dump_outputs, {"hidden": out, "next_ids": ids})

    session.close()
    manager.shutdown()
    # release the workers, then spin down
    boot.store("bench_done", "client", True, time.time() + 600)
    p50 = sorted(step_ms)[len(step_ms) // 2]
    result = {
        "metric": f"decode tokens/sec, {args.model} greedy, serving stack over RCCL/xGMI",
        "value": round(global_batch * args.steps / elapsed, 2),
        "unit": "tokens/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": round(elapsed * 1000 / args.steps, 3),
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": "bfloat16" if cfg.torch_dtype == "bfloat16" else cfg.torch_dtype,
        "data": "synthetic",
        "config": {
            "model": args.model,
            "global_batch": global_batch,
            "seq_len": args.prompt,
            "parallelism": f"swarm-pp{world}",
            "p50_step_ms": round(p50, 3),
        },
    }
    print(json.dumps(result))
    time.sleep(1.0)
    server.shutdown()
    boot.shutdown()
    channels.disable()
    if dist.is_initialized():
        dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=16)
    ap.add_argument("--model", default="llama-3-8b")
    ap.add_argument("--batch-per-gpu", type=int, default=32)
    ap.add_argument("--prompt", type=int, default=2048,
                    help="prompt length prefillled before the timed decode steps")
    ap.add_argument("--device", default=None, help="override (e.g. cpu for tests)")
    ap.add_argument("--micro-batches", type=int, default=0)
    ap.add_argument("--tp", type=int, default=1,
                    help="tensor-parallel degree within the pipeline (world %% tp == 0)")
    ap.add_argument("--tp-mode", default="tensor", choices=["tensor", "expert"],
                    help="what the intra-stage group shards: tensor dims "
                         "(llama TP) or MoE experts (mixtral EP)")
    ap.add_argument("--mode", default="pipeline", choices=["pipeline", "swarm"],
                    help="pipeline = raw RCCL pipeline stages (flagship); "
                         "swarm = the full decentralized serving stack "
                         "(DHT + sessions + handler) over the same device plane")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last one "
                         "returned as DIR/<name>.npy (float32, <= 64 MB)")
    ap.add_argument("--full", action="store_true",
                    help="also run every measurement beyond the headline "
                         "figure (none today: a plain run already does only "
                         "setup, warmup, the timed steps and the result line)")
    args = ap.parse_args()

    if args.mode == "swarm":
        run_swarm(args)
        return

    import torch.distributed as dist
    from bloombee_amd.parallel.pipeline import PipelineStage, init_distributed

    device = init_distributed("cpu" if args.device == "cpu" else "auto")
    if args.device:
        device = args.device
    rank = dist.get_rank() if dist.is_initialized() else 0
    world = dist.get_world_size() if dist.is_initialized() else 1
    assert world == args.gpus or not dist.is_initialized(), \
        f"world {world} != --gpus {args.gpus}"
    on_gpu = device.startswith("cuda")

    global_batch = args.batch_per_gpu * world
    session_len = args.prompt + args.steps + args.warmup + 8
    assert session_len <= stage_max_pos(args.model), (
        f"prompt+steps {session_len} exceeds the model's "
        f"max_position_embeddings — shorten --prompt or --steps")
    # KV budget: whole session for every sequence on every rank (page-rounded)
    kv_tokens = global_batch * ((session_len + 15) // 16 + 1) * 16 + 1024

    stage = PipelineStage(args.model, device, global_batch,
                          micro_batches=args.micro_batches,
                          kv_max_tokens=kv_tokens, max_session_len=session_len,
                          tp=args.tp, tp_mode=args.tp_mode)

    gen = torch.Generator().manual_seed(42)
    V = stage.config.vocab_size
    ids = None
    if rank == 0:
        prompt = torch.randint(0, V, (global_batch, args.prompt), generator=gen)
    # ---- prefill (untimed setup; chunked to bound activation memory) ----
    CH = 512
    for c0 in range(0, args.prompt, CH):
        chunk = None
        if rank == 0:
            chunk = prompt[:, c0:c0 + CH]
        ids = stage.prefill_round(chunk, min(CH, args.prompt - c0))

    # ---- warmup ----
    for _ in range(args.warmup):
        ids = stage.decode_round(ids if rank == 0 else None)

    if dist.is_initialized():
        dist.barrier()
    if on_gpu:
        torch.cuda.synchronize()

    step_ms = []
    t0 = time.monotonic()
    if on_gpu and rank == 0:
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(args.steps + 1)]
        ev[0].record()
    for s in range(args.steps):
        ids = stage.decode_round(ids if rank == 0 else None)
        if on_gpu and rank == 0:
            ev[s + 1].record()
    if on_gpu:
        torch.cuda.synchronize()
    if dist.is_initialized():
        dist.barrier()
    if on_gpu:
        torch.cuda.synchronize()
    t1 = time.monotonic()
    elapsed = t1 - t0
    if dist.is_initialized():
        e = torch.tensor([elapsed])
        dist.all_reduce(e, op=dist.ReduceOp.MAX)
        elapsed = float(e)

    if rank == 0:
        if on_gpu:
            step_ms = [ev[i].elapsed_time(ev[i + 1]) for i in range(args.steps)]
        else:
            step_ms = [elapsed / args.steps * 1000] * args.steps
        p50 = sorted(step_ms)[len(step_ms) // 2]
        tokens_per_s = global_batch * args.steps / elapsed
        result = {
            "metric": f"decode tokens/sec, {args.model} greedy, pipeline over RCCL/xGMI",
            "value": round(tokens_per_s, 2),
            "unit": "tokens/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(elapsed * 1000 / args.steps, 3),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "bfloat16" if stage.config.torch_dtype == "bfloat16" else stage.config.torch_dtype,
            "data": "synthetic",
            "config": {
                "model": args.model,
                "global_batch": global_batch,
                "seq_len": args.prompt,
                "parallelism": (f"pp{world // args.tp}x"
                                f"{'ep' if args.tp_mode == 'expert' else 'tp'}"
                                f"{args.tp}" if args.tp > 1 else f"pp{world}"),
                "micro_batches": stage.M,
                "p50_step_ms": round(p50, 3),
            },
        }
        if args.dump_outputs:
            # decode_round hands its caller the next token of every sequence
            dump_outputs(args.dump_outputs, {"next_ids": ids})
        print(json.dumps(result))
    if dist.is_initialized():
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
