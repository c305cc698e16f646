"""CPU (-m "not gpu"): host logic, the C-ABI library's exports, sharding + table broadcast over gloo (world_size 2).
No compute call needs a GPU here; nothing in the product routes through the oracle."""
import ctypes
import os
import re
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import kit_golden
import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol():
    """libaa_interp.so loads without a GPU and exports exactly what include/aa_interp.h declares."""
    from interpolate_antialiasing_amd import _lib

    L = _lib.load()
    header = open(_lib.HEADER_PATH).read()
    declared = set(re.findall(r"^\s*(?:const\s+char\s*\*\s*|size_t\s+|int\s+)(aa_[a-z0-9_]+)\s*\(", header, flags=re.M))
    assert declared, "no declarations parsed"
    assert declared == set(_lib.EXPORTS), (declared ^ set(_lib.EXPORTS))
    for sym in declared:
        assert hasattr(L, sym), sym
    assert L.aa_abi_version() == 3
    assert L.aa_device_count() >= 0  # 0 on the CPU-only build box, never throws
    assert _lib.strerror(-2).startswith("dtype")


def test_ksize_host_arithmetic_matches_oracle():
    """aa_table_ksize replicates s2.2:207-210 (and Pillow's ceil(support)*2+1) on the host."""
    from interpolate_antialiasing_amd import _lib

    L = _lib.load()
    for filt, fid in (("linear", 0), ("cubic", 1), ("box", 2)):
        for n_in, n_out in [(906, 320), (438, 196), (1024, 224), (438, 1200), (906, 1200), (64, 64), (61, 1), (3, 2), (5, 7)]:
            assert L.aa_table_ksize(fid, _lib.TABLE_F32, n_in, n_out, 0, 0.0) == oracle.ksize(filt, n_in, n_out, False, np.float32)
            assert L.aa_table_ksize(fid, _lib.TABLE_F64, n_in, n_out, 0, 0.0) == oracle.ksize(filt, n_in, n_out, False, np.float64)
            assert L.aa_table_ksize(fid, _lib.TABLE_F32, n_in, n_out, 1, 0.0) == oracle.ksize(filt, n_in, n_out, True, np.float32)
            assert L.aa_table_ksize(fid, _lib.TABLE_PIL, n_in, n_out, 0, 0.0) == oracle.pil_coeffs(filt, n_in, n_out)[0]
    assert L.aa_table_ksize(7, _lib.TABLE_F32, 8, 4, 0, 0.0) == -1  # AA_ERR_BAD_FILTER
    assert L.aa_table_ksize(0, _lib.TABLE_F32, 0, 4, 0, 0.0) == -4  # AA_ERR_BAD_SHAPE
    assert L.aa_table_ksize(0, _lib.TABLE_PIL, 8, 4, 1, 0.0) == -2  # Pillow has no align_corners
    # table sizes: header + bounds + padded weights (+ scatter records for Pillow tables)
    assert L.aa_table_bytes(_lib.TABLE_F32, 320, 7) == 64 + ((8 * 320 + 15) // 16) * 16 + 320 * 7 * 4 + 32 * 320  # + gather records
    assert L.aa_table_build_bytes(0, _lib.TABLE_PIL, 438, 196, 0, 0.0) == L.aa_table_bytes(_lib.TABLE_PIL, 196, 7) + 32 * (438 + 1)
    assert L.aa_table_build_bytes(1, _lib.TABLE_F32, 1024, 224, 0, 0.0) == L.aa_table_bytes(_lib.TABLE_F32, 224, 21) + 32 * (1024 + 1)
    assert L.aa_table_build_bytes(0, _lib.TABLE_F64, 438, 196, 0, 0.0) == L.aa_table_bytes(_lib.TABLE_F64, 196, 7) + 64 * (438 + 1)  # double-weight records


def test_argument_errors_without_gpu():
    """Same wording as ATen's upsample_2d_common_check / the reference's dispatch errors; raised before any device work."""
    from interpolate_antialiasing_amd import _lib
    from interpolate_antialiasing_amd import extension_interpolate as aa

    x = torch.zeros(1, 3, 8, 8)
    with pytest.raises(RuntimeError, match="Input and output sizes should be greater than 0"):
        aa.linear_forward(x, [0, 4])
    with pytest.raises(RuntimeError, match="It is expected input_size equals to 4"):
        aa.cubic_forward(x[0], [4, 4])
    with pytest.raises(RuntimeError, match="It is expected output_size equals to 2"):
        aa.nearest_forward(x, [4, 4, 4])
    with pytest.raises(NotImplementedError, match="not implemented for 'Int'"):
        aa.linear_forward(x.int(), [4, 4])
    with pytest.raises(RuntimeError, match="It is expected output_size equals to 3"):
        aa.linear_forward_nd(torch.zeros(1, 2, 4, 4, 4), [4, 4])
    with pytest.raises(NotImplementedError, match="not implemented for 'Byte'"):
        aa.linear_forward_nd(torch.zeros(1, 2, 9, dtype=torch.uint8), [4])
    # the product is the HIP path only: CPU tensors fail loudly, nothing falls back to a CPU implementation
    with pytest.raises(_lib.AAInterpError, match="no CPU implementation"):
        aa.linear_forward(x, [4, 4])
    with pytest.raises(RuntimeError, match="Expected grad_output to have the same shape as output"):
        aa.linear_backward(torch.zeros(1, 3, 5, 7), [5, 8], [1, 3, 12, 17])
    with pytest.raises(_lib.AAInterpError, match="no CPU implementation"):
        aa.linear_backward(torch.zeros(1, 3, 5, 7), [5, 7], [1, 3, 12, 17])
    assert aa.forward is aa.linear_forward  # legacy export of every other step
    with pytest.raises(ValueError):
        aa.set_uint8_mode("nearest")
    # torch.ops surface exists with the reference's names
    for name in ("linear_forward", "nearest_forward", "cubic_forward", "linear_backward", "forward"):
        assert hasattr(torch.ops.extension_interpolate, name)
    # shape inference without a device
    y = torch.ops.extension_interpolate.linear_forward(torch.zeros(2, 3, 8, 8, device="meta"), [4, 5], False)
    assert tuple(y.shape) == (2, 3, 4, 5)


def test_product_does_not_import_the_oracle():
    """The package must never depend on oracle/ (a product path through the checker would void the parity claims)."""
    pkg = os.path.join(ROOT, "interpolate_antialiasing_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                src = open(os.path.join(dirpath, f)).read()
                assert not re.search(r"^\s*(import|from)\s+oracle\b", src, flags=re.M), f
                assert "liboracle" not in src and "aa_oracle" not in src, f


def test_shard_range_partitions_exactly():
    from interpolate_antialiasing_amd import sharding

    for total in (0, 1, 7, 8, 1000, 8192):
        for world in (1, 2, 3, 8):
            spans = [sharding.shard_range(total, r, world) for r in range(world)]
            assert spans[0][0] == 0 and spans[-1][1] == total
            for (a0, a1), (b0, b1) in zip(spans, spans[1:]):
                assert a1 == b0 and a0 <= a1
            sizes = [b - a for a, b in spans]
            assert max(sizes) - min(sizes) <= 1
    assert sharding.shard_range(8192, 3, 8) == (3072, 4096)  # config 3: 1024 images per GPU
    with pytest.raises(ValueError):
        sharding.shard_range(8, 2, 2)


def test_weight_table_pack_unpack_roundtrip():
    from interpolate_antialiasing_amd import _lib
    from interpolate_antialiasing_amd.tables import WeightTable

    buf, k, mt = kit_golden.pack_table_numpy("linear", 906, 320)
    t = WeightTable(torch.from_numpy(buf), 0, _lib.TABLE_F32, 906, 320, k, mt)
    xmin, xsize, w = t.unpack()
    ko, xo, so, wo = oracle.weights("linear", 906, 320)
    assert np.array_equal(xmin, xo) and np.array_equal(xsize, so) and np.array_equal(w, wo)
    t2 = WeightTable.from_meta(t.meta(), t.buf.clone())
    assert (t2.filter, t2.kind, t2.in_size, t2.out_size, t2.ksize, t2.max_taps) == (0, 1, 906, 320, k, mt)
    with pytest.raises(_lib.AAInterpError):
        t.axis()  # a CPU-resident table cannot be handed to the kernels


_WORKER = r'''
import os, sys, numpy as np, torch, torch.distributed as dist
sys.path.insert(0, sys.argv[1])
from interpolate_antialiasing_amd import _lib, sharding
from interpolate_antialiasing_amd.tables import WeightTable
sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
from kit_golden import pack_table_numpy
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
dist.init_process_group("gloo", rank=rank, world_size=world)
# rank 0 owns the table; everyone else receives it with the single broadcast the path has
t = None
if rank == 0:
    buf, k, mt = pack_table_numpy("linear", 438, 196)
    t = WeightTable(torch.from_numpy(buf), 0, _lib.TABLE_F32, 438, 196, k, mt)
got = sharding.broadcast_table(t, src=0, device=torch.device("cpu"))
ref, k, mt = pack_table_numpy("linear", 438, 196)
assert np.array_equal(got.buf.numpy(), ref) and got.ksize == k and got.max_taps == mt and got.in_size == 438
# batch shard of config 3 + the bench's reductions
a, b = sharding.shard_range(8192, rank, world)
assert b - a == 8192 // world
x = torch.arange(10)
assert sharding.shard_batch(x, rank, world).tolist() == list(range(*sharding.shard_range(10, rank, world)))
assert sharding.reduce_sum_int(b - a) == 8192
assert abs(sharding.reduce_max_seconds(0.5 + rank) - (0.5 + world - 1)) < 1e-12
dist.barrier()
dist.destroy_process_group()
print("worker", rank, "ok")
'''


def test_table_broadcast_and_sharding_gloo_world2(tmp_path):
    """The N>1 path (one process per rank, table broadcast, shard, reductions) with the gloo backend on CPU."""
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    script = tmp_path / "worker.py"
    script.write_text(_WORKER)
    procs = []
    for rank in range(2):
        env = dict(os.environ, RANK=str(rank), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, str(script), ROOT], env=env, stdout=subprocess.PIPE,
                                      stderr=subprocess.STDOUT, text=True))
    outs = [p.communicate(timeout=180)[0] for p in procs]
    for rank, (p, out) in enumerate(zip(procs, outs)):
        assert p.returncode == 0, out
        assert f"worker {rank} ok" in out


def test_bench_launcher_starts_n_ranks():
    """`python bench.py --gpus N` (no torch.distributed.run around it) starts N fresh rank processes itself, before any GPU
    call: each rank sees its RANK / WORLD_SIZE / MASTER_* and the bench line's skeleton carries n_gpus = N and
    global_batch = N x batch.  --launch-dry-run makes the ranks exit before touching a GPU, so this runs on the CPU box."""
    import json

    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--batch", "64", "--launch-dry-run"],
                         capture_output=True, text=True, timeout=300, env={k: v for k, v in os.environ.items()
                                                                           if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")})
    assert out.returncode == 0, out.stderr
    lines = [json.loads(l) for l in out.stdout.splitlines() if l.startswith("{")]
    assert [l["rank"] for l in lines] == [0, 1] and all(l["world"] == 2 and l["dry_run"] for l in lines)
    assert lines[0]["master"] == lines[1]["master"] and lines[0]["master"].startswith("127.0.0.1:")
    assert lines[0]["n_gpus"] == 2 and lines[0]["config"]["global_batch"] == 128 and lines[0]["scaling"] == "weak"
    # under torch.distributed.run the environment carries the world: the same script is then a rank, not a launcher
    env = dict(os.environ, RANK="1", LOCAL_RANK="1", WORLD_SIZE="4", MASTER_ADDR="127.0.0.1", MASTER_PORT="1")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "4", "--launch-dry-run"], capture_output=True,
                         text=True, timeout=300, env=env)
    assert out.returncode == 0 and json.loads(out.stdout)["rank"] == 1 and json.loads(out.stdout)["world"] == 4
    # a world that contradicts --gpus is refused, naming the right commands
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "8", "--launch-dry-run"], capture_output=True,
                         text=True, timeout=300, env=env)
    assert out.returncode != 0 and "torch.distributed.run" in out.stderr


def test_bench_launcher_survives_chatty_and_failing_ranks():
    """The launcher drains every rank concurrently (stderr of ranks > 0 into files, stdout by threads) and polls all of them:
    a rank that writes a megabyte to stderr cannot block on a pipe, and when one rank fails the others are killed instead of
    waiting in a collective until the driver's timeout (round-2 advisor finding on launch_ranks)."""
    import json
    import time

    base = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "3", "--launch-dry-run"], capture_output=True, text=True,
                         timeout=300, env=dict(base, AA_BENCH_DRYRUN_HOOK="chatty"))
    assert out.returncode == 0, out.stderr[-2000:]
    assert [json.loads(l)["rank"] for l in out.stdout.splitlines() if l.startswith("{")] == [0, 1, 2]
    t0 = time.time()
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--launch-dry-run"], capture_output=True, text=True,
                         timeout=300, env=dict(base, AA_BENCH_DRYRUN_HOOK="fail1"))
    assert out.returncode != 0 and "rank 1 exited with 3" in out.stderr and time.time() - t0 < 120, (out.returncode, out.stderr[-500:])


def test_bench_dump_outputs_sample(tmp_path):
    """--dump-outputs writes float32 NCHW images of the timed output: all of a small batch; of a large one the same seeded
    sample of bench.DUMP_IMAGES images on every run, in batch order, which at the headline shape stays under 64 MB."""
    import bench

    assert bench.DUMP_IMAGES * 3 * bench.H_OUT * bench.W_OUT * 4 <= 64 << 20
    small = torch.randint(0, 256, (5, 4, 6, 3), dtype=torch.uint8).permute(0, 3, 1, 2)  # channels_last, as the bench's output
    bench.dump_outputs(str(tmp_path / "a"), small)
    got = np.load(tmp_path / "a" / "output.npy")
    assert got.dtype == np.float32 and np.array_equal(got, small.float().numpy())
    big = torch.arange(200, dtype=torch.uint8).view(200, 1, 1, 1).expand(200, 3, 2, 2).contiguous()  # image i holds the value i
    bench.dump_outputs(str(tmp_path / "b"), big)
    bench.dump_outputs(str(tmp_path / "c"), big)
    b, c = np.load(tmp_path / "b" / "output.npy"), np.load(tmp_path / "c" / "output.npy")
    assert b.shape == (bench.DUMP_IMAGES, 3, 2, 2) and np.array_equal(b, c)
    picked = b[:, 0, 0, 0]
    assert np.all(np.diff(picked) > 0) and np.all(b == picked[:, None, None, None])


def test_headline_kernel_keeps_six_waves_per_simd(tmp_path):
    """Occupancy regression guard (no GPU needed: read from the built code object).  The headline kernel — uint8 channels_last,
    3 channels, 6-tap windows, 2 open output rows, non-negative weights, periodic slot phases — must stay within 80 VGPRs
    (6 waves per SIMD: single-strip workgroups fill 24 wave slots per CU).  At 81 the launch heuristic falls back to
    5-strip workgroups and the bench loses ~8 % (round 2: an innocent emit branch hoisted its address arithmetic)."""
    import shutil

    objdump, readelf = "/opt/rocm/lib/llvm/bin/llvm-objdump", "/opt/rocm/lib/llvm/bin/llvm-readelf"
    obj = os.path.join(ROOT, "interpolate_antialiasing_amd", "csrc", "aa_fused_u8_v3_c3.o")
    if not (os.path.exists(objdump) and os.path.exists(readelf) and os.path.exists(obj)):
        pytest.skip("needs the ROCm LLVM tools and the built object")
    local = tmp_path / "c3.o"
    shutil.copy(obj, local)
    subprocess.run([objdump, "--offloading", str(local)], check=True, capture_output=True, cwd=tmp_path)
    cos = [f for f in os.listdir(tmp_path) if "gfx950" in f]
    assert cos, os.listdir(tmp_path)
    notes = subprocess.run([readelf, "--notes", str(tmp_path / cos[0])], check=True, capture_output=True, text=True).stdout
    m = re.search(r"\.name:\s+\S*fused_u8_nhwc_v3_kernelILi3ELi6ELi8ELb0ELi2ELb1ELb1ELb0E\S*\n(?:.*\n){0,40}?\s+\.vgpr_count:\s+(\d+)", notes)
    if m is None:  # field order differs: search backwards as well
        blocks = notes.split("- .agpr_count")
        hit = [b for b in blocks if "fused_u8_nhwc_v3_kernelILi3ELi6ELi8ELb0ELi2ELb1ELb1ELb0E" in b]
        assert hit, "headline kernel not found in the code object"
        m = re.search(r"\.vgpr_count:\s+(\d+)", hit[0])
    assert m is not None
    assert int(m.group(1)) <= 80, f"headline kernel uses {m.group(1)} VGPRs (> 80: 5 waves per SIMD)"
