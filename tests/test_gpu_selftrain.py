"""GPU: the bit-row kernels of csrc/selftrain.hip against numpy (selftrain_cases.py), `load_self_train_bits` against
`load_self_train_masks`, and one self-training round end to end through the tools.  Every comparison is exact."""
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

import dataset_cases as D
import selftrain_cases as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _to_dev(bits, device):
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int64)).to(device)


def _to_host(bits):
    return bits.cpu().numpy().view(np.uint64)


# ------------------------------------------------------------------------------------------------- pack / unpack
@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 7, 64, 130])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 127, 4099])
def test_pack_unpack_round_trip(device, n, k):
    """bits == numpy_pack, count == popcounts, the tail of the last word is zero in a buffer that held 0xFF, and
    `mask_bits_to_columns` gives the table back (f32, uint8 and bool; into a wider table at a column offset)."""
    from unscene3d_amd import _lib, ops

    rng = np.random.default_rng(1000 * n + k)
    m = rng.random((n, k)) < rng.uniform(0.05, 0.95, k)
    m[:, k // 2] = n % 2 == 0                                    # one full or empty column
    vals = np.where(m, rng.integers(1, 256, (n, k)), 0).astype(np.uint8)       # non-zero = set, not only 1
    ref = S.numpy_pack(m)
    W = (n + 63) // 64

    bits, count = ops.mask_columns_to_bits(torch.from_numpy(vals).to(device))
    assert bits.shape == (k, W) and np.array_equal(_to_host(bits), ref)
    assert count.dtype == torch.int32 and np.array_equal(count.cpu().numpy(), m.sum(0))
    b2, c2 = ops.mask_columns_to_bits(torch.from_numpy(m).to(device))          # bool input
    assert torch.equal(b2, bits) and torch.equal(c2, count)

    dirty = torch.full((k, W), -1, dtype=torch.int64, device=device)           # every byte 0xFF
    dcount = torch.full((k,), -1, dtype=torch.int32, device=device)
    src = torch.from_numpy(vals).to(device)
    _lib.check(_lib.lib.usc_mask_columns_to_bits(src.data_ptr(), n, k, dirty.data_ptr(), dcount.data_ptr(),
                                                 torch.cuda.current_stream().cuda_stream), "usc_mask_columns_to_bits")
    got = _to_host(dirty)
    assert np.array_equal(got, ref)
    if n % 64:
        assert not (got[:, -1] >> np.uint64(n % 64)).any()
    assert np.array_equal(dcount.cpu().numpy(), m.sum(0))
    assert np.array_equal(ops.mask_bits_count(bits, n).cpu().numpy(), m.sum(0))

    for dtype, np_dtype in ((torch.float32, np.float32), (torch.uint8, np.uint8), (torch.bool, bool)):
        back = ops.mask_bits_to_columns(bits, n, dtype=dtype)
        assert back.dtype == dtype and np.array_equal(back.cpu().numpy(), m.astype(np_dtype))
    rows = list(rng.permutation(k)[:max(1, k // 2)])
    wide = torch.full((n, len(rows) + 5), 7.0, device=device)
    ops.mask_bits_to_columns(bits, n, rows=rows, out=wide, col0=3)
    exp = np.full((n, len(rows) + 5), 7.0, np.float32)
    exp[:, 3:3 + len(rows)] = m[:, rows]
    assert np.array_equal(wide.cpu().numpy(), exp)


@pytest.mark.gpu
def test_pack_of_a_table_with_no_columns_and_unpack_of_more_rows_than_a_chunk(device):
    from unscene3d_amd import ops

    bits, count = ops.mask_columns_to_bits(torch.zeros((70, 0), dtype=torch.bool, device=device))
    assert bits.shape == (0, 2) and count.shape == (0,)
    rng = np.random.default_rng(5)
    m = rng.random((130, 300)) < 0.4                             # 300 rows: two LDS rounds of the unpack
    back = ops.mask_bits_to_columns(_to_dev(S.numpy_pack(m), device), 130, dtype=torch.uint8)
    assert np.array_equal(back.cpu().numpy(), m.astype(np.uint8))


# ---------------------------------------------------------------------------------------------------------- gather
@pytest.mark.gpu
@pytest.mark.parametrize("m,n,k", [(100, 333, 7), (4099, 1001, 130), (65, 63, 1)])
def test_gather_equals_pack_of_the_indexed_table(device, m, n, k):
    from unscene3d_amd import ops

    rng = np.random.default_rng(m + n + k)
    table = rng.random((m, k)) < 0.4
    ind = rng.integers(0, m, n)                                  # with repeats; some rows never chosen
    ind[0], ind[-1] = m - 1, 0
    ref = table[ind]
    dst, count = ops.mask_bits_gather(_to_dev(S.numpy_pack(table), device), m, torch.from_numpy(ind).to(device))
    assert np.array_equal(_to_host(dst), S.numpy_pack(ref))
    assert np.array_equal(count.cpu().numpy(), ref.sum(0))
    with pytest.raises(RuntimeError, match="out of range"):
        ops.mask_bits_gather(_to_dev(S.numpy_pack(table), device), m, torch.tensor([0, m], device=device))


# ----------------------------------------------------------------------------------------------------------- merge
@pytest.fixture(scope="module")
def packed_cases(device):
    out = {}
    for name, st, cov in S.merge_cases():
        bits = S.numpy_pack(st)
        out[name] = (st.shape[0], _to_dev(bits, device), torch.from_numpy(S.numpy_popcount(bits)).to(device),
                     _to_dev(S.numpy_pack(cov[:, None])[0], device))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("branch", ["lds", "global"])
def test_merge_equals_the_host_rule(device, packed_cases, branch):
    """Every case x max_add x kp: picked, n_added, fresh and the final cover == numpy_merge; the planted ties are
    refused; a second run gives the same bytes.  `global`: the LDS limit set to zero words, so the cover stays in
    global memory."""
    from unscene3d_amd import _lib, ops

    default = _lib.lib.usc_selftrain_merge_lds_words(0 if branch == "global" else -1)
    try:
        for name, (n, st, total, cov) in packed_cases.items():
            W = (n + 63) // 64
            for max_add in S.MAX_ADD:
                for kp in S.KP:
                    exp = S.merge_expectations()[(name, max_add, kp)]
                    runs = []
                    for _ in range(2):
                        fg = cov.clone()
                        fresh, picked, n_added = ops.selftrain_merge(st[:kp].contiguous(), total[:kp].contiguous(), n,
                                                                     fg, max_add)
                        runs.append((fresh, picked, n_added, fg))
                    fresh, picked, n_added, fg = runs[0]
                    a = len(exp["picked"])
                    where = (name, max_add, kp)
                    assert int(n_added) == a, where
                    assert picked.cpu().tolist() == exp["picked"] + [-1] * (max_add - a), where
                    assert fresh.shape == (max_add, W)
                    assert np.array_equal(_to_host(fresh[:a]), S.numpy_pack(exp["fresh"]).reshape(a, W)), where
                    assert not fresh[a:].any(), where
                    assert np.array_equal(_to_host(fg), S.numpy_pack(exp["covered"][:, None])[0]), where
                    for x, y in zip(runs[0], runs[1]):
                        assert torch.equal(x, y), where
        tie = S.merge_expectations()[("planted4099", 5, 100)]
        assert 2 not in tie["picked"] and 4 not in tie["picked"] and 0 in tie["picked"] and 5 in tie["picked"]
    finally:
        _lib.lib.usc_selftrain_merge_lds_words(default)
    assert _lib.lib.usc_selftrain_merge_lds_words(-1) == default == 7168


# ------------------------------------------------------------------------------------------------ reader functions
def _scene(n=4099, K=6, seed=3):
    """Points in columns of 16 whose feet follow a Z-order curve: a run of consecutive indices (the planted
    instances, the initial cover) is compact in x and y and passes the reader's extent filter."""
    rng = np.random.default_rng(seed)
    idx = np.arange(n)
    cell = idx // 16
    cx = sum(((cell >> (2 * b)) & 1) << b for b in range(8))
    cy = sum(((cell >> (2 * b + 1)) & 1) << b for b in range(8))
    grid = np.stack([cx, cy, idx % 16], 1)
    pts = np.hstack([grid * 0.05, rng.random((n, 9))]).astype(np.float32)      # [N,12] like a scene file
    st, cov = S._planted(n, seed)
    soft = rng.random((n, K)).astype(np.float32) * cov[:, None]                 # soft masks, non-zero where covered
    soft[:, 1] = 0
    return pts, soft, st[:, :30]


@pytest.mark.gpu
@pytest.mark.parametrize("cloud", ["same", "permuted"])
def test_load_self_train_bits_equals_load_self_train_masks(device, cloud):
    """Values and dtype, for the same cloud and for a permuted, jittered one (1-NN transfer), `drop_original` on and
    off, no original masks at all, soft f32 and bool input, several caps; then `as_device=True` ->
    `mask_tables_device` gives the numpy route's table and keep list."""
    from unscene3d_amd.datasets.freemask import load_self_train_bits, load_self_train_masks, mask_tables_device

    pts, soft, st = _scene()
    n = pts.shape[0]
    if cloud == "same":
        st_cloud, st_masks = pts[:, :3].copy(), st
    else:
        rng = np.random.default_rng(9)
        perm = rng.permutation(n)[:n - 37]                         # another length, some points without a twin
        st_cloud = (pts[perm, :3] + rng.uniform(-1e-3, 1e-3, (n - 37, 3))).astype(np.float32)
        st_masks = st[perm]
    bits = S.numpy_pack(st_masks)
    seg = (np.arange(n) // 7).astype(np.float32)
    inputs = {"soft": soft, "bool": soft > 0.5, "none": np.zeros((n, 0), np.float32)}
    took_some = kept_new = False
    for kind, fm in inputs.items():
        for drop in (False, True):
            for cap in (5, 2, 0):
                ref = load_self_train_masks(pts, fm, st_cloud, st_masks, cap, drop_original=drop, device=device)
                got = load_self_train_bits(pts, fm, st_cloud, bits, cap, drop_original=drop, device=device)
                where = (kind, drop, cap)
                assert got.dtype == ref.dtype and got.shape == ref.shape, where
                assert np.array_equal(got, ref), where
                took_some |= ref.shape[1] > (0 if drop else fm.shape[1])
                dev_t = load_self_train_bits(pts, fm, st_cloud, bits, cap, drop_original=drop, device=device,
                                             as_device=True)
                assert dev_t.is_cuda and dev_t.dtype == torch.float32 and dev_t.shape == ref.shape
                assert np.array_equal(dev_t.cpu().numpy(), ref.astype(np.float32)), where
                t_ref, keep_ref = mask_tables_device(pts[:, :3], ref, seg, device=device)
                t_got, keep_got = mask_tables_device(pts[:, :3], dev_t, seg, device=device)
                assert keep_got == keep_ref, where
                assert (t_ref is None and t_got is None) or torch.equal(t_got, t_ref), where
                kept_new |= any(j >= (0 if drop else fm.shape[1]) for j in keep_ref)
                if ref.shape[1] > 2:                               # the reader's max_num_gt_instances slice
                    t_ref, keep_ref = mask_tables_device(pts[:, :3], ref[:, :2], seg, device=device)
                    t_got, keep_got = mask_tables_device(pts[:, :3], dev_t[:, :2], seg, device=device)
                    assert keep_got == keep_ref and ((t_ref is None and t_got is None) or torch.equal(t_got, t_ref))
    assert took_some and kept_new              # merged columns were added, and some of them reach the table
    with pytest.raises(ValueError, match="bits must be uint64"):
        load_self_train_bits(pts, soft, st_cloud, bits[:, :-1], device=device)


@pytest.mark.gpu
def test_save_for_freemask_bits_and_both(device, tmp_path):
    """`bits` writes the cloud and the bit rows only, `both` all three; the unpacked bit rows are the bool table; a
    scene without instances writes a [0, W] array."""
    from unscene3d_amd.trainer.postprocess import save_for_freemask

    rng = np.random.default_rng(2)
    coords = rng.standard_normal((4099, 3)).astype(np.float32)
    masks = rng.random((4099, 9)) < 0.2
    save_for_freemask(str(tmp_path / "bits"), "scene0000_00", coords, torch.from_numpy(masks).to(device), "bits")
    save_for_freemask(str(tmp_path / "both"), "scene0000_00", coords, torch.from_numpy(masks).to(device), "both")
    save_for_freemask(str(tmp_path / "none"), "scene0000_00", coords, torch.zeros((4099, 0), dtype=torch.bool,
                                                                                device=device), "bits")
    assert sorted(os.listdir(tmp_path / "bits" / "freemasks")) == ["scene0000_00_cloud.npy", "scene0000_00_masks_bits.npy"]
    assert sorted(os.listdir(tmp_path / "both" / "freemasks")) == ["scene0000_00_cloud.npy", "scene0000_00_masks.npy",
                                                                  "scene0000_00_masks_bits.npy"]
    for d in ("bits", "both"):
        b = np.load(tmp_path / d / "freemasks" / "scene0000_00_masks_bits.npy")
        assert b.dtype == np.uint64 and b.shape == (9, 65) and np.array_equal(b, S.numpy_pack(masks))
        assert np.array_equal(np.load(tmp_path / d / "freemasks" / "scene0000_00_cloud.npy"), coords)
    assert np.array_equal(np.load(tmp_path / "both" / "freemasks" / "scene0000_00_masks.npy"), masks)
    empty = np.load(tmp_path / "none" / "freemasks" / "scene0000_00_masks_bits.npy")
    assert empty.dtype == np.uint64 and empty.shape == (0, 65)


# ------------------------------------------------------------------------------------------------------ end to end
def _same_items(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert type(x) is type(y)
        if isinstance(x, torch.Tensor):
            assert x.dtype == y.dtype and x.device == y.device and torch.equal(x, y)
        elif isinstance(x, np.ndarray):
            assert x.dtype == y.dtype and np.array_equal(x, y)
        else:
            assert x == y


@pytest.mark.gpu
def test_one_round_from_scan_directories_through_the_tools(device, tmp_path):
    """Two 40-side scans -> tools/dataset_from_scans.py -> tools/train.py --steps 2 -> tools/export_round.py --format
    both -> the readers -> tools/train.py --self-train-dir on the bit rows.  A randomly initialised network decides
    what the export holds, so this asserts equality only: the unpacked bit rows are the bool table of the same scene,
    the files carry the names the reader looks for, a reader over the bit rows alone returns the items of a reader
    over the bool tables alone (device tables on and off), and the second training run returns 0 with finite losses."""
    from unscene3d_amd.datasets.freemask import FreeMaskSceneReader, entries_from_database, load_color_mean_std

    names = ("scene0000_00", "scene0001_00")
    for i, name in enumerate(names):
        scan = D.write_scan(str(tmp_path / "scans"), name, seed=20 + i, side=40)
        D.write_pseudo(str(tmp_path / "pm"), name, scan, seed=20 + i, K=5, compact=True)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    run = lambda *a: subprocess.run([sys.executable, *a], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    data = str(tmp_path / "data")
    r = run("tools/dataset_from_scans.py", "--scans", str(tmp_path / "scans"), "--pseudo", str(tmp_path / "pm"),
            "--out", data)
    assert r.returncode == 0, r.stderr[-2000:]
    r = run("tools/train.py", "--data-dir", data, "--steps", "2", "--out", str(tmp_path / "run"))
    assert r.returncode == 0, r.stderr[-2000:]
    st_dir = tmp_path / "self_train"
    r = run("tools/export_round.py", "--data-dir", data, "--checkpoint", str(tmp_path / "run" / "last.ckpt"),
            "--out", str(st_dir), "--format", "both")
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["scenes"] + len(line["skipped"]) == 2 and line["format"] == "both" and line["checkpoint_step"] == 2
    assert line["scenes"] == 2, line                               # a file per scene
    assert sorted(line["masks_per_scene"]) == list(names)

    entries = entries_from_database(os.path.join(data, "train_database.yaml"))
    only = {"bits": tmp_path / "only_bits", "npy": tmp_path / "only_npy"}
    written = 0
    for e, name in zip(entries, names):
        stem = f"scene{os.path.splitext(os.path.basename(e['filepath']))[0]}"
        assert stem == name                                         # ScanNet layout: the reader's scene name
        base = st_dir / "freemasks"
        cloud, masks = np.load(base / f"{stem}_cloud.npy"), np.load(base / f"{stem}_masks.npy")
        bits = np.load(base / f"{stem}_masks_bits.npy")
        assert masks.dtype == bool and masks.shape[0] == cloud.shape[0] == e["file_len"]
        assert masks.shape[1] == line["masks_per_scene"][name]
        assert bits.dtype == np.uint64 and bits.shape == (masks.shape[1], (masks.shape[0] + 63) // 64)
        assert np.array_equal(S.numpy_unpack(bits, masks.shape[0]), masks)
        assert np.array_equal(bits, S.numpy_pack(masks))            # the tail bits too
        for kind, suffixes in (("bits", ("_cloud.npy", "_masks_bits.npy")), ("npy", ("_cloud.npy", "_masks.npy"))):
            os.makedirs(only[kind] / "freemasks", exist_ok=True)
            for s in suffixes:
                shutil.copy(base / f"{stem}{s}", only[kind] / "freemasks" / f"{stem}{s}")
        written += sum(os.path.getsize(base / f"{stem}{s}") for s in ("_cloud.npy", "_masks.npy", "_masks_bits.npy"))
    assert line["bytes_written"] == written

    stats = load_color_mean_std(os.path.join(data, "color_mean_std.yaml"))
    for dev_tables in (False, True):
        readers = [FreeMaskSceneReader(entries, color_mean_std=stats, add_normals=False, add_raw_coordinates=True,
                                       device=str(device), device_tables=dev_tables, load_self_train_data=True,
                                       self_train_data_dir=str(only[kind])) for kind in ("bits", "npy")]
        for i in range(len(entries)):
            _same_items(readers[0][i], readers[1][i])

    r = run("tools/train.py", "--data-dir", data, "--self-train-dir", str(only["bits"]), "--steps", "2")
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["steps"] == 2 and line["skipped"] == 0
    assert len(line["losses_per_step"]) == 2 and np.isfinite(np.array(line["losses_per_step"])).all()
