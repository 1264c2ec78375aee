"""CPU-side tests: the C-ABI library loads and exports every symbol the header declares, the
Python mirror has the reference's surface (names, signatures, state_dict keys, init behaviour),
the host logic (schedules, sharding, flat buffers) is right, and the product path refuses to
compute without a GPU (no CPU fallback)."""
import ctypes
import inspect
import math
import os
import sys

import numpy as np
import pytest
import torch

from oracle import onet_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol():
    from onet_amd import _lib
    protos = _lib.parse_header()
    assert len(protos) >= 30
    lib = ctypes.CDLL(_lib.LIBPATH) if os.path.exists(_lib.LIBPATH) else _lib.load()
    for name in protos:
        assert hasattr(lib, name), name
    lib2 = _lib.load()
    assert lib2.onet_abi_version() == 4
    assert lib2.onet_jsd_nparts() > 0
    assert lib2.onet_conv_wgrad_ws_bytes(32, 64, 64, 256, 256, 3) > 0


def test_bad_arguments_return_error_codes_not_crashes():
    from onet_amd import _lib
    lib = _lib.load()
    rc = lib.onet_conv_fwd(None, 0, None, None, 0, None, 1, 1, 1, 1, 1, 3, None)
    assert rc == -1 and b"null" in lib.onet_last_error()
    with pytest.raises(_lib.OnetHipError, match="ks must be 1 or 3"):
        _lib.call("onet_conv_fwd", 8, 64, 8, 8, 64, None, 1, 1, 1, 8, 8, 5, None)


def test_module_surface_matches_reference_signatures():
    import Onet_vanilla_20240606 as ov
    assert list(inspect.signature(ov.DoubleConv.__init__).parameters)[1:] == ["in_channels", "out_channels", "mid_channels"]
    assert list(inspect.signature(ov.Down.__init__).parameters)[1:] == ["in_channels", "out_channels"]
    sig = inspect.signature(ov.Up.__init__).parameters
    assert list(sig)[1:] == ["in_channels", "out_channels", "bilinear"] and sig["bilinear"].default is True
    sig = inspect.signature(ov.UNet.__init__).parameters
    assert [(k, v.default) for k, v in list(sig.items())[1:]] == [("n_channels", 1), ("n_classes", 1), ("binit", False), ("bilinear", False)]
    sig = inspect.signature(ov.Onet.__init__).parameters
    assert [(k, v.default) for k, v in list(sig.items())[1:]] == [("in_chns", 1), ("binit", False), ("bshare", True)]
    for meth in ("forward", "predict_label", "get_label", "jensen_shannon_divergence", "log1pexp", "compute_loss"):
        assert callable(getattr(ov.Onet, meth))
    assert list(inspect.signature(ov.Onet.compute_loss).parameters)[1:] == ["Lt", "St", "Ld", "Sd"]
    assert list(inspect.signature(ov.Onet.jensen_shannon_divergence).parameters)[1:] == ["Li", "Si", "Sprime"]


@pytest.mark.parametrize("in_chns,bshare", [(1, True), (3, True), (1, False)])
def test_state_dict_keys_and_shapes_match_reference_layout(in_chns, bshare):
    from onet_amd import Onet
    m = Onet(in_chns=in_chns, binit=True, bshare=bshare)
    sd = m.state_dict()
    ref = orc.onet_state_dict(in_chns, 1981, bshare)
    assert list(sd.keys()) == list(ref.keys())
    assert len(sd) == 232
    for k in sd:
        assert tuple(sd[k].shape) == tuple(ref[k].shape), k
        assert sd[k].dtype == ref[k].dtype, k
    assert (m.dwnu is m.topu) == bshare
    n = sum(p.numel() for p in m.parameters())
    assert n == (31036416 if in_chns == 1 else 31036416 + 2 * 64 * 9) * (1 if bshare else 2)
    assert len(list(m.parameters())) == (62 if bshare else 124)
    m.load_state_dict(ref)      # reference-format checkpoints load
    assert m.bias == 0 and isinstance(m.softmax, torch.nn.Softmax2d)


def test_init_follows_reference_rules():
    """binit: Kaiming-normal(fan_in, relu) on every nn.Conv2d, BN weight 1 / bias 0; ConvTranspose2d keeps
    torch's default init with a NON-zero bias."""
    from onet_amd import Onet
    torch.manual_seed(0)
    m = Onet(1, binit=True)
    w = m.topu.down2.maxpool_conv[1].double_conv[3].weight
    assert abs(float(w.std()) - math.sqrt(2.0 / (256 * 9))) < 0.02 * math.sqrt(2.0 / (256 * 9))
    bn = m.topu.inc.double_conv[1]
    assert float(bn.weight.min()) == 1.0 and float(bn.bias.abs().max()) == 0.0
    up = m.topu.up1.up
    assert isinstance(up, torch.nn.ConvTranspose2d) and not isinstance(up, torch.nn.Conv2d)
    bound = 1.0 / math.sqrt(512 * 4)
    assert float(up.weight.abs().max()) <= bound + 1e-6 and float(up.bias.abs().max()) > 0


def test_cpu_tensor_is_refused_loudly():
    from onet_amd import Onet
    m = Onet(1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(torch.zeros(2, 1, 16, 16))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.compute_loss(torch.zeros(1, 64, 4, 4), torch.zeros(1, 1, 4, 4), torch.zeros(1, 64, 4, 4), torch.zeros(1, 1, 4, 4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.predict_label(torch.zeros(1, 2, 4, 4))


def test_product_does_not_import_the_oracle():
    import re
    pkg = os.path.join(ROOT, "onet_amd")
    for fn in os.listdir(pkg):
        if fn.endswith(".py"):
            src = open(os.path.join(pkg, fn)).read()
            assert not re.search(r"^\s*(from|import)\s+oracle", src, flags=re.M), fn
    assert not re.search(r"^\s*(from|import)\s+oracle", open(os.path.join(ROOT, "Onet_vanilla_20240606.py")).read(), flags=re.M)


def test_sim_lr_schedule_matches_reference_loop():
    from onet_amd.trainer import sim_lr
    lr, seen = 5e-6, []
    for epoch in range(301):
        seen.append(lr)
        if epoch % 100 == 0 and epoch > 0:     # TS:248-249
            lr *= 0.5
    assert [sim_lr(e) for e in range(301)] == pytest.approx(seen, rel=1e-12)


def test_cosine_schedule_matches_torch_scheduler():
    from onet_amd.trainer import cosine_warm_restarts_lr
    p = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.Adam([p], lr=1e-4)
    sch = torch.optim.lr_scheduler.CosineAnnealingWarmRestarts(opt, T_0=300, T_mult=2, eta_min=1e-6)
    for epoch in range(1000):
        assert cosine_warm_restarts_lr(epoch) == pytest.approx(opt.param_groups[0]["lr"], rel=1e-9), epoch
        opt.step()
        sch.step()


def test_shard_batch_and_flat_buffers():
    from onet_amd.trainer import FlatAdam, shard_batch
    X = torch.arange(8 * 3).reshape(8, 3)
    assert torch.equal(torch.cat([shard_batch(X, r, 4) for r in range(4)]), X)
    with pytest.raises(ValueError):
        shard_batch(X, 0, 3)
    lin = torch.nn.Sequential(torch.nn.Linear(5, 3), torch.nn.Linear(3, 2))
    ref = [p.detach().clone() for p in lin.parameters()]
    opt = FlatAdam(lin, lr=1e-3)
    assert opt.numel % 4 == 0 and all(o % 4 == 0 for o in opt.offsets)
    for p, r, off in zip(lin.parameters(), ref, opt.offsets):
        assert torch.equal(p.detach(), r)
        assert p.data_ptr() == opt.flat.data_ptr() + 4 * off
        assert p.grad.data_ptr() == opt.gflat.data_ptr() + 4 * off
    lin(torch.ones(4, 5)).sum().backward()
    assert float(opt.gflat.abs().sum()) > 0            # autograd accumulated INTO the flat buffer
    lin.zero_grad()                                     # set_to_none: grads detach from the flat buffer
    lin(torch.ones(4, 5)).sum().backward()
    opt.zero_grad()
    assert float(opt.gflat.abs().sum()) == 0
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        opt.step()                                      # the fused Adam kernel has no CPU path


def test_synthetic_clutter_generator():
    from onet_amd import data
    X, lab = data.make_clutter_batch(2, 64, 64, seed=3, with_labels=True)
    assert X.shape == (2, 1, 64, 64) and X.dtype == np.float32 and lab.shape == (2, 64, 64)
    assert float(X.min()) == 0.0 and float(X.max()) == 1.0
    X2 = data.make_clutter_batch(2, 64, 64, seed=3)
    assert np.array_equal(X, X2)
    # K-distributed amplitude is heavier-tailed than Rayleigh: scale-free moment ratio E[a^4]/E[a^2]^2 > 2
    a = data.k_clutter_frame(np.random.Generator(np.random.PCG64(1)), 256)
    assert np.mean(a ** 4) / np.mean(a ** 2) ** 2 > 2.1


def test_up_block_oracle_vs_reference_golden():
    """oracle.upsample_cat (convT and bilinear, F.pad path) pinned to the real reference's Up block."""
    import zlib
    for tag, bilinear in (("convT_pad", False), ("bilinear_pad", True)):
        g = np.load(os.path.join(ROOT, "tests", "golden", f"up_{tag}.npz"))
        h, w, H, W, _ = [int(v) for v in g["meta"]]
        names = (["up.weight", "up.bias"] if not bilinear else [])
        mid = 64
        shapes = {"up.weight": (128, 64, 2, 2), "up.bias": (64,)}
        st = {}
        for k in names:
            rng = np.random.Generator(np.random.PCG64([3, zlib.crc32(k.encode())]))
            shp = shapes[k]
            if len(shp) == 4:
                st["blk." + k] = torch.from_numpy((rng.standard_normal(shp) * np.sqrt(2.0 / (shp[1] * 4))).astype(np.float32))
            else:
                st["blk." + k] = torch.from_numpy((0.1 * rng.standard_normal(shp)).astype(np.float32))
        x1 = orc.det_input(2, 64 if bilinear else 128, h, w, seed=21)
        x2 = orc.det_input(2, 64, H, W, seed=22)
        cat = orc.upsample_cat(x1, x2, st, "blk", bilinear=bilinear)
        assert cat.shape == (2, 128, H, W)
        # first conv of the block (in -> mid) on the concat must reproduce the reference's y after BN/ReLU x2:
        for idx, (ci, co) in ((0, (128, mid)), (3, (mid, 64))):
            for suffix, shp in ((f"conv.double_conv.{idx}.weight", (co, ci, 3, 3)),):
                rng = np.random.Generator(np.random.PCG64([3, zlib.crc32(suffix.encode())]))
                st["w%d" % idx] = torch.from_numpy((rng.standard_normal(shp) * np.sqrt(2.0 / (ci * 9))).astype(np.float32))
            b = idx + 1
            for nm in ("weight", "bias", "running_mean", "running_var"):
                key = f"conv.double_conv.{b}.{nm}"
                rng = np.random.Generator(np.random.PCG64([3, zlib.crc32(key.encode())]))
                if nm == "running_var":
                    v = 1 + 0.1 * np.abs(rng.standard_normal((co,)))
                elif nm == "weight":
                    v = 1 + 0.1 * rng.standard_normal((co,))
                else:
                    v = 0.1 * rng.standard_normal((co,))
                st[f"bn{idx}.{nm}"] = torch.from_numpy(v.astype(np.float32))
        y = cat
        for idx in (0, 3):
            y = torch.nn.functional.conv2d(y, st["w%d" % idx], None, 1, 1)
            y = torch.relu(torch.nn.functional.batch_norm(y, st[f"bn{idx}.running_mean"].clone(), st[f"bn{idx}.running_var"].clone(),
                                                          st[f"bn{idx}.weight"], st[f"bn{idx}.bias"], True, 0.1, 1e-5))
        np.testing.assert_allclose(y.numpy(), g["y"], rtol=1e-4, atol=1e-5)


def test_reference_wire_formats(tmp_path):
    """checkpoint {'net','epoch'|'save_epoch'} and the sim-clutter .pt dict schema."""
    from onet_amd import Onet, io
    from onet_amd import data
    m = Onet(1, binit=True)
    io.save_checkpoint(m, tmp_path / "a.pytorch", 7)
    io.save_checkpoint(m, tmp_path / "b.pytorch", 9, zy3=True)
    ck = torch.load(tmp_path / "a.pytorch")
    assert sorted(ck.keys()) == ["epoch", "net"] and len(ck["net"]) == 232
    assert sorted(torch.load(tmp_path / "b.pytorch").keys()) == ["net", "save_epoch"]
    m2 = Onet(1)
    assert io.load_checkpoint(m2, tmp_path / "a.pytorch") == 7
    assert io.load_checkpoint(m2, tmp_path / "b.pytorch") == 9
    assert torch.equal(m2.topu.up1.up.bias, m.topu.up1.up.bias)
    X, lab = data.make_clutter_batch(3, 32, 32, seed=5, with_labels=True)
    io.save_simclutter_pt(tmp_path / "r.pt", X, lab, [0, 1, 2])
    d = torch.load(tmp_path / "r.pt")
    assert sorted(d.keys()) == ["psnr", "rayleigh_imgs", "rayleigh_labels"] and d["rayleigh_imgs"].shape == (3, 1, 32, 32)
    imgs, labels, snrs = io.load_simclutter_pt(tmp_path / "r.pt")
    assert imgs.dtype == torch.float32 and labels.shape == (3, 32, 32) and snrs.tolist() == [0, 1, 2]
    tr, te = io.split_train_test(10)
    assert len(tr) == 9 and len(te) == 1 and sorted(np.concatenate([tr, te]).tolist()) == list(range(10))


def test_bench_self_launch_relays_the_ranks_exit_code():
    """`python bench.py --gpus 2` outside a launcher starts its ranks as a child `torch.distributed.run` (no GPU call in the
    parent) and hands back THEIR exit code: on this GPU-less box every rank fails loudly (no device), so must the parent --
    and it must not have imported torch.cuda state or the HIP library itself to find that out."""
    import subprocess
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    env["ONET_FORCE_LOCAL_RANK"] = "0"          # the one-GPU rehearsal switch waives the device-count preflight (tested below)
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: tests/test_gpu_dist.py::test_bench_launches_its_own_ranks covers the success path")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0",
                          "--batch", "2", "--size", "32", "--no-cpu-baseline"], cwd=ROOT, env=env, capture_output=True,
                         text=True, timeout=300)
    assert out.returncode != 0
    assert "torch.distributed.run" in out.stderr and "--nproc-per-node 2" in out.stderr
    assert not [ln for ln in out.stdout.splitlines() if ln.startswith("{")]


def test_bench_preflight_refuses_more_gpus_than_the_node_has():
    """`python bench.py --gpus 64` on a box with fewer GPUs: exit code 2 and a message naming both numbers, before any rank or
    collective is started."""
    import subprocess
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "ONET_FORCE_LOCAL_RANK")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "64", "--no-cpu-baseline"], cwd=ROOT, env=env,
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 2, (out.returncode, out.stderr[-1000:])
    assert "--gpus 64" in out.stderr and "nothing was launched" in out.stderr
    assert "torch.distributed.run" not in out.stderr


def test_bench_parent_is_gpu_free_before_the_launch_decision():
    """bench.py imports neither torch nor onet_amd at module level (the launcher decision comes first)."""
    import ast
    tree = ast.parse(open(os.path.join(ROOT, "bench.py")).read())
    top = [n for n in tree.body if isinstance(n, (ast.Import, ast.ImportFrom))]
    names = {a.name.split(".")[0] for n in top if isinstance(n, ast.Import) for a in n.names} | \
            {n.module.split(".")[0] for n in top if isinstance(n, ast.ImportFrom) and n.module}
    assert not ({"torch", "onet_amd", "oracle"} & names), names


def test_bench_bracket_options_need_full():
    """--bracket-all / --mfma-events-only only shape the roofline, which a plain run does not measure: refused without --full."""
    import subprocess
    for opt in ("--bracket-all", "--mfma-events-only"):
        out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), opt], cwd=ROOT, capture_output=True, text=True,
                             timeout=120)
        assert out.returncode == 2 and "need --full" in out.stderr, (opt, out.stderr[-1000:])


def test_bench_dump_outputs_format(tmp_path, monkeypatch):
    """bench.dump_outputs on a CPU model: float32 arrays within 64 MB, and the parameter / gradient sample takes the same
    positions in every run (two builds are compared output for output)."""
    import bench
    from onet_amd import Onet
    monkeypatch.setattr(bench, "torch", torch)         # bench.main() imports torch into the module
    m = Onet(in_chns=1, binit=True, bshare=True)
    for i, p in enumerate(m.parameters()):
        p.grad = torch.full_like(p, float(i))
    bench.dump_outputs(str(tmp_path / "a"), m, torch.tensor(0.5))
    bench.dump_outputs(str(tmp_path / "b"), m, torch.tensor(0.5))
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["bn_running_stats.npy", "grads_sample.npy", "loss.npy", "params_sample.npy"]
    arrays = {n: np.load(tmp_path / "a" / n) for n in names}
    assert all(a.dtype == np.float32 for a in arrays.values())
    assert sum(a.nbytes for a in arrays.values()) <= 64 * 2 ** 20
    assert arrays["params_sample.npy"].size == bench.DUMP_SAMPLE and float(arrays["loss.npy"][0]) == 0.5
    for n in names:
        assert np.array_equal(arrays[n], np.load(tmp_path / "b" / n)), n
    flat_g = torch.cat([p.grad.reshape(-1) for p in m.parameters()]).numpy()
    assert set(np.unique(arrays["grads_sample.npy"])) <= set(np.unique(flat_g))


def test_zy3_dict_reader(tmp_path):
    """`io.load_zy3_dict` on a file with the schema the reference's ZY-3 loaders read (dataloader/zy3_cloud_thumbnailv5_20240304.py:
    92-122 `torch.load` of `{image_id: {'true_color': tensor [3,H,W], 'mask': tensor [H,W]}}`; the Dataset indexes
    `list(data_dict.keys())`, :139-141, and its test branch hands out the stored tensors unchanged, :163-169): ids in the
    file's order (not sorted), float32 stacks, values untouched, uint8 / float64 sources converted.  The real dataset is
    absent (.MISSING_LARGE_BLOBS), so BASELINE configs[4]'s IoU parity itself cannot be run -- this pins the reader only."""
    from onet_amd import io
    rng = np.random.Generator(np.random.PCG64(3))
    d = {}
    for key, dt in (("ZY3_0007", torch.float32), ("ZY3_0002", torch.float64), ("scene_b", torch.uint8)):
        rgb = torch.from_numpy(rng.random((3, 24, 20))).to(torch.float32)
        d[key] = {"true_color": (rgb * 255).to(dt) if dt == torch.uint8 else rgb.to(dt),
                  "mask": torch.from_numpy((rng.random((24, 20)) > 0.7)).to(dt)}
    torch.save(d, tmp_path / "zy3.pt")
    ids, X, M = io.load_zy3_dict(tmp_path / "zy3.pt")
    assert ids == ["ZY3_0007", "ZY3_0002", "scene_b"]                  # the reference's order: insertion, not sorted
    assert X.shape == (3, 3, 24, 20) and M.shape == (3, 24, 20) and X.dtype == M.dtype == torch.float32
    for i, k in enumerate(ids):
        assert torch.equal(X[i], d[k]["true_color"].to(torch.float32)) and torch.equal(M[i], d[k]["mask"].to(torch.float32))
    assert set(M.unique().tolist()) <= {0.0, 1.0}


def test_batch_counters_are_collected_and_applied_once():
    """ops.counting_batches (UNet.forward: the 18 BatchNorm num_batches_tracked increments of a pass in one multi-tensor launch):
    increments made inside the block land when it ends -- also when it raises -- and immediately outside of one."""
    from onet_amd import ops
    a, b = torch.zeros((), dtype=torch.int64), torch.zeros((), dtype=torch.int64)
    with ops.counting_batches():
        ops.count_batches(a, 2)
        ops.count_batches(b, 2)
        assert int(a) == 0 and int(b) == 0
        with ops.counting_batches():                     # nested (an unshared second U-Net inside another model's pass)
            ops.count_batches(a, 1)
        assert int(a) == 1
    assert int(a) == 3 and int(b) == 2
    ops.count_batches(b, 1)
    assert int(b) == 3
    with pytest.raises(ValueError):
        with ops.counting_batches():
            ops.count_batches(a, 1)
            raise ValueError("a unit refused its input")
    assert int(a) == 4
