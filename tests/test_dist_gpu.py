"""Multi-GPU through the C-ABI itself: two ranks, each with its own handle on its
own GPU, run a native forward of their shard into bit-packed masks and exchange them with the
library's RCCL all-gather (unet_comm_get_unique_id / unet_comm_init / unet_allgather) -- the path a
C host without torch.distributed takes.  Each rank's gathered batch must equal a single-process
forward of the whole batch on GPU 0, bit for bit.  Needs two GPUs (skipped on the one-GPU box;
the gloo tests in test_dist_cpu.py cover the sharding logic there)."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rank(rank, world, uid, x, sd, q):
    sys.path.insert(0, os.path.join(REPO, "tw-invoice-unet-ocr-llm_amd"))
    from unet_mi355x import native
    from unet_mi355x.model import UNet
    try:
        dev = torch.device("cuda", rank)
        torch.cuda.set_device(dev)
        m = UNet(3, 3, compute_dtype="mixed")
        m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
        m = m.to(dev).eval()
        h = m.native_handle(dev)
        n = x.shape[0] // world
        xs = torch.from_numpy(x[rank * n:(rank + 1) * n]).to(dev)
        h.reserve(n, x.shape[2], x.shape[3])
        send = torch.empty((n, 3, x.shape[2], x.shape[3] // 8), dtype=torch.uint8, device=dev)
        recv = torch.empty((world * n,) + tuple(send.shape[1:]), dtype=torch.uint8, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        h.comm_init(rank, world, uid)
        h.forward(xs, None, send, native.MASK_BITS, stream)
        h.allgather(send, recv, stream)
        torch.cuda.synchronize(dev)
        h.comm_destroy()
        q.put((rank, recv.cpu().numpy()))
        m.close()
    except Exception as e:  # pragma: no cover - reported to the parent
        q.put((rank, repr(e)))


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two GPUs (the one-GPU box runs the gloo tests)")
def test_two_rank_native_forward_and_rccl_allgather():
    sys.path.insert(0, os.path.join(REPO, "tw-invoice-unet-ocr-llm_amd"))
    from unet_mi355x import native, synthetic as syn
    from unet_mi355x.model import UNet
    world = 2
    x = syn.invoice_pages(11, 4, 128, 128, 3)
    sd = {k: np.asarray(v) for k, v in syn.make_state_dict(0, 3, 3, "pretrained").items()}
    uid = native.Handle.comm_unique_id()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_rank, args=(r, world, uid, x, sd, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = dict(q.get(timeout=300) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
    for r in range(world):
        assert not isinstance(got[r], str), got[r]
    m = UNet(3, 3, compute_dtype="mixed")
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    m = m.to("cuda:0").eval()
    with torch.no_grad():
        ref = m.forward_masks(torch.from_numpy(x).to("cuda:0"), packed=True).cpu().numpy()
    m.close()
    for r in range(world):
        assert np.array_equal(got[r], ref), f"rank {r}'s gathered masks differ from the one-process forward"


def _gloo_rank(rank, world, port, x, sd, q):
    """One rank of the one-GPU, two-process run: its own handle on cuda:0, the bench's sharding and
    exchange step (dist.ShardedSegmenter: shard_bounds + all_gather_rows) over gloo, and the bench's
    timing loop (dist.timed_steps: barriers + the MAX-over-ranks all-reduce)."""
    sys.path.insert(0, os.path.join(REPO, "tw-invoice-unet-ocr-llm_amd"))
    import torch.distributed as tdist
    from unet_mi355x import dist as udist
    from unet_mi355x.model import UNet
    try:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        tdist.init_process_group("gloo", rank=rank, world_size=world)
        dev = torch.device("cuda", 0)
        m = UNet(3, 3, compute_dtype="mixed")
        m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
        m = m.to(dev).eval()

        def seg(local):   # the native forward of this rank's shard; the gloo exchange runs on the host
            with torch.no_grad():
                return m.forward_masks(local.to(dev), packed=True).cpu()
        step = udist.ShardedSegmenter(seg)
        xt = torch.from_numpy(x)
        got = step(xt)
        elapsed, per_step = udist.timed_steps(lambda: step(xt), 2, 1, torch.cuda.synchronize, torch.device("cpu"))
        q.put((rank, (got.numpy(), elapsed, len(per_step))))
        m.close()
        tdist.destroy_process_group()
    except Exception as e:  # pragma: no cover - reported to the parent
        q.put((rank, repr(e)))


def test_two_ranks_share_one_gpu_gloo_exchange(monkeypatch):
    """Multi-rank on the one-GPU box: two processes, each with its own native handle on cuda:0, run
    their contiguous shards of a ragged global batch (5 pages: 3 + 2) and exchange the bit-packed masks
    with the bench's sharding/exchange code over gloo; every rank's gathered batch equals a
    one-process forward of the whole batch bit for bit, and the timing loop's MAX-over-ranks
    all-reduce agrees on both ranks.  (RCCL refuses two ranks on one device; the RCCL exchange itself
    is test_two_rank_native_forward_and_rccl_allgather, on two GPUs.)  The shards (N = 3, 2) would take
    the small-batch split-K plan, which sums in another order than the N = 5 forward: it is off here
    (UNET_MI355X_KSPLIT=0, inherited by the ranks), as in the bench's multi-GPU shapes."""
    import socket
    monkeypatch.setenv("UNET_MI355X_KSPLIT", "0")
    sys.path.insert(0, os.path.join(REPO, "tw-invoice-unet-ocr-llm_amd"))
    from unet_mi355x import synthetic as syn
    from unet_mi355x.model import UNet
    world = 2
    x = syn.invoice_pages(13, 5, 128, 128, 3)
    sd = {k: np.asarray(v) for k, v in syn.make_state_dict(0, 3, 3, "pretrained").items()}
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_gloo_rank, args=(r, world, port, x, sd, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = dict(q.get(timeout=150) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
    for r in range(world):
        assert not isinstance(got[r], str), got[r]
    m = UNet(3, 3, compute_dtype="mixed")
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    m = m.to("cuda:0").eval()
    with torch.no_grad():
        ref = m.forward_masks(torch.from_numpy(x).to("cuda:0"), packed=True).cpu().numpy()
    m.close()
    for r in range(world):
        masks, elapsed, n_steps = got[r]
        assert np.array_equal(masks, ref), f"rank {r}'s gathered masks differ from the one-process forward"
        assert n_steps == 2 and elapsed > 0
    assert got[0][1] == got[1][1], "the MAX-over-ranks elapsed time differs between ranks"


def _world8_rank(rank, world, port, out_dir, q):
    """One rank of BASELINE config 4's workload on the one-GPU box: bench.py's own runner, sharding
    (make_leg: rank r's contiguous shard of the global batch, forwards in chunks of the reserved
    workspace) and timing loop (time_leg: barriers, per-step marks, the MAX-over-ranks all-reduce), with
    the exchange -- all_gather_into_tensor of the bit-packed masks -- over gloo instead of RCCL."""
    import argparse
    import hashlib
    sys.path.insert(0, REPO)
    import torch.distributed as tdist
    try:
        import bench
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        tdist.init_process_group("gloo", rank=rank, world_size=world)
        dev = torch.device("cuda", 0)
        torch.cuda.set_device(dev)
        runner = bench.NativeRunner(argparse.Namespace(channels=3, weights="pretrained", dtype="mixed"), dev, world)
        runner.reserve(W8_CHUNK, 512)
        leg = bench.make_leg(runner, rank, world, W8_GLOBAL, None, W8_SEED, 512, 3, dev, W8_CHUNK)
        t = bench.time_leg(leg, 1, 1, torch.cuda.synchronize, dev, per_step_events=True)
        comp = bench.over_ranks(float(t["compute_ms"][0]), dev)
        rows = leg["gather"].rows().cpu().numpy()
        if rank == 0:
            np.save(os.path.join(out_dir, "gathered.npy"), rows)
        q.put((rank, (hashlib.sha256(rows.tobytes()).hexdigest(), t["elapsed"], comp, leg["n_local"],
                      t["allgather_ms"][0])))
        runner.model.close()
        tdist.destroy_process_group()
    except Exception as e:  # pragma: no cover - reported to the parent
        import traceback
        q.put((rank, repr(e) + traceback.format_exc()))


W8_GLOBAL, W8_CHUNK, W8_SEED = 1024, 32, 3000


@pytest.mark.timeout(600)
def test_world_eight_ranks_config4_on_one_gpu(tmp_path):
    """BASELINE config 4 (global batch 1024 at 512^2 over 8 ranks: 128 images each) with 8 fresh rank
    processes on cuda:0: every rank runs its shard through bench.py's make_leg / time_leg (chunked
    forwards of 32 images, so eight workspaces fit one GPU's HBM) and all-gathers the bit-packed masks
    over gloo.  Every rank's gathered 1024 masks equal a one-process forward of the whole batch (here in
    forwards of 256: another batch size than the ranks') bit for bit, and the MAX-over-ranks step time
    and compute time agree on all ranks.  Only the transport (gloo vs RCCL over xGMI) differs from the
    8-GPU run."""
    import socket
    sys.path.insert(0, REPO)
    import bench
    from unet_mi355x import dist as udist, native
    world = 8
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_world8_rank, args=(r, world, port, str(tmp_path), q)) for r in range(world)]
    for p in procs:
        p.start()
    try:
        got = dict(q.get(timeout=420) for _ in range(world))
    finally:
        for p in procs:
            p.join(timeout=60)
            if p.is_alive():
                p.kill()
    for r in range(world):
        assert not isinstance(got[r], str), got[r]
    assert [got[r][3] for r in range(world)] == [128] * 8
    assert len({got[r][0] for r in range(world)}) == 1, "ranks gathered different masks"
    assert len({got[r][1] for r in range(world)}) == 1, "the MAX-over-ranks step time differs between ranks"
    assert len({got[r][2] for r in range(world)}) == 1, "the MAX/MIN compute times differ between ranks"
    cmax, cmin = got[0][2]
    assert 0 < cmin <= cmax <= 1e3 * got[0][1] + 1e-3
    gathered = np.load(tmp_path / "gathered.npy")
    assert gathered.shape == (W8_GLOBAL, 3, 512, 64)
    # the one-process forward of the same global batch: rank r's pages are gen_pages(seed + r, shard)
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in bench.syn.make_state_dict(0, 3, 3, "pretrained").items()}
    from unet_mi355x.model import UNet
    m = UNet(3, 3, compute_dtype="mixed")
    m.load_state_dict(sd)
    m = m.to("cuda:0").eval()
    pages = np.concatenate([bench.gen_pages(W8_SEED + r, 128, 512, 3) for r in range(world)])
    h = m.native_handle(torch.device("cuda", 0))
    h.reserve(256, 512, 512)
    stream = torch.cuda.current_stream().cuda_stream
    ref = torch.empty((W8_GLOBAL, 3, 512, 64), dtype=torch.uint8, device="cuda:0")
    for i in range(0, W8_GLOBAL, 256):
        h.forward(torch.from_numpy(pages[i:i + 256]).to("cuda:0"), None, ref[i:i + 256], native.MASK_BITS, stream)
    ref = ref.cpu().numpy()
    m.close()
    assert udist.shard_bounds(W8_GLOBAL, 7, world) == (896, 1024)
    assert np.array_equal(gathered, ref), "the 8 ranks' gathered masks differ from the one-process forward"


_WORLD1_SCRIPT = r"""
import os, sys, json
import numpy as np, torch, torch.distributed as dist
sys.path.insert(0, os.path.join(sys.argv[1], "tw-invoice-unet-ocr-llm_amd"))
sys.path.insert(0, sys.argv[1])
import bench
from unet_mi355x import dist as udist, native, synthetic as syn
from unet_mi355x.model import UNet
os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=sys.argv[2])
dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)      # bench.py --dist
m = UNet(3, 3, compute_dtype="mixed")
m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in syn.make_state_dict(0, 3, 3, "pretrained").items()})
m = m.to(dev).eval()
h = m.native_handle(dev)
x = torch.from_numpy(syn.invoice_pages(17, 6, 128, 128, 3)).to(dev)
h.reserve(6, 128, 128)
stream = torch.cuda.current_stream(dev).cuda_stream
g = udist.MaskGather(6, (3, 128, 16), torch.uint8, dev, rank=0, world=1, collective=True)
assert g.out.data_ptr() != g.send.data_ptr()
g.out.fill_(0xAB)
seg = lambda xl, ml: h.forward(xl, None, ml, native.MASK_BITS, stream)
udist.sharded_mask_step(seg, x, g)                   # forward into the send buffer + RCCL all-gather
ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
t, per = udist.timed_steps(lambda: udist.sharded_mask_step(seg, x, g), 3, 1, torch.cuda.synchronize, dev,
                           collective=True)          # barriers + the device MAX all-reduce
torch.cuda.synchronize()
ref = torch.empty_like(g.send)
seg(x, ref)
torch.cuda.synchronize()
print(json.dumps({"equal": bool(torch.equal(g.out, ref)), "sent_equal": bool(torch.equal(g.send, ref)),
                  "elapsed": t, "steps": len(per)}))
dist.destroy_process_group()
m.close()
"""


def test_world_one_nccl_exchange_equals_forward(tmp_path):
    """The N > 1 exchange on the one-GPU box: an nccl (RCCL) process group of world size 1 with
    device_id, the preallocated MaskGather forced to run all_gather_into_tensor into its separate
    receive buffer, and dist.timed_steps' barriers + device MAX all-reduce.  The gathered masks equal
    a plain forward bit for bit.  Run in a child process (one process group, one RCCL communicator)."""
    import json
    import socket
    import subprocess
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    script = tmp_path / "world1.py"
    script.write_text(_WORLD1_SCRIPT)
    p = subprocess.run([sys.executable, str(script), REPO, str(port)], capture_output=True, text=True, timeout=150)
    assert p.returncode == 0, p.stderr[-3000:]
    out = json.loads(p.stdout.strip().splitlines()[-1])
    assert out["sent_equal"] and out["equal"], out
    assert out["steps"] == 3 and out["elapsed"] > 0


def test_bench_dist_world_one_line(tmp_path):
    """bench.py --dist --gpus 1 (nccl at world size 1): the line names the exchange and reports the
    all-gather's own time per step (HIP events around the collective), which is a small share of the
    step; the detail record holds the per-step all-gather times."""
    import json
    import subprocess
    detail = tmp_path / "detail.json"
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    p = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--dist", "--batch", "8",
                        "--size", "256", "--steps", "4", "--warmup", "2", "--full", "--no-cpu-baseline", "--no-latency",
                        "--no-fp32", "--no-cfg5", "--no-strong", "--detail-out", str(detail)],
                       cwd=REPO, env=env, capture_output=True, text=True, timeout=170)
    assert p.returncode == 0, p.stderr[-3000:]
    out = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
    assert out["config"]["exchange"] == "all_gather_into_tensor" and out["n_gpus"] == 1
    assert out["allgather_ms"] is not None and 0 < out["allgather_ms"] < out["ms_per_step"]
    assert out["roofline"]["allgather_ms"] == out["allgather_ms"]
    rec = json.loads(detail.read_text())
    assert len(rec["detail"]["allgather_ms"]) == 4
