"""bench.py --dump-outputs: the sample positions and the files it writes, on host tensors (no GPU needed)."""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench  # noqa: E402


def test_sample_index_is_fixed_sorted_distinct_and_in_bounds():
    assert (bench._sample_index(np, 10, 16) == np.arange(10)).all()
    for n, cap in ((1000, 1000), (1001, 1000), (8 << 30, 1 << 21), (3 * (1 << 20) + 7, 1 << 20)):
        a, b = bench._sample_index(np, n, cap), bench._sample_index(np, n, cap)
        assert a.size == min(n, cap) and (a == b).all()
        assert a.dtype == np.int64 and a[0] >= 0 and a[-1] < n and (np.diff(a) > 0).all()


def _fake_outputs(n, bb, total):
    K = (n + bb - 1) // bb
    g = torch.Generator().manual_seed(1)
    blk = types.SimpleNamespace(
        payload=torch.randint(0, 256, (n,), dtype=torch.uint8, generator=g),
        comp_size=torch.randint(0, 1 << 31, (K,), dtype=torch.int32, generator=g),
        comp_off=torch.arange(K, dtype=torch.int64) * (3 << 30),
        code_lengths=torch.randint(0, 33, (K, 256), dtype=torch.uint8, generator=g),
        status=torch.zeros(K, dtype=torch.int32), total=torch.tensor([total], dtype=torch.int64))
    t_out = torch.randint(0, 256, (n,), dtype=torch.uint8, generator=g)
    return blk, t_out, torch.zeros(K, dtype=torch.int32), torch.full((K,), -1, dtype=torch.int64)


def test_dump_outputs_writes_every_array_exactly_and_within_the_cap(tmp_path):
    env = types.SimpleNamespace(np=np, torch=torch)
    n, bb, total = (1 << 21) + 4096, 4096, 1 << 20
    blk, t_out, dstatus, derrpos = _fake_outputs(n, bb, total)
    written = bench._dump_outputs(env, str(tmp_path), blk, t_out, dstatus, derrpos, n)
    assert set(written) == set(bench.DUMP_CAPS)
    files = sorted(os.listdir(tmp_path))
    assert files == sorted(nm + ".npy" for nm in bench.DUMP_CAPS)
    assert sum(os.path.getsize(os.path.join(tmp_path, f)) for f in files) <= bench.DUMP_MAX_BYTES
    ld = {nm: np.load(os.path.join(tmp_path, nm + ".npy")) for nm in bench.DUMP_CAPS}
    for nm, a in ld.items():
        assert a.dtype in (np.float32, np.float64), nm
        assert a.size == written[nm][0] <= bench.DUMP_CAPS[nm], nm
    # the one sampled array here: payload positions past `total` read -1, the others are the bytes themselves
    idx = bench._sample_index(np, n, bench.DUMP_CAPS["payload"])
    pay = blk.payload.numpy()[idx].astype(np.float32)
    pay[idx >= total] = -1
    assert written["payload"] == [idx.size, n] and (ld["payload"] == pay).all()
    assert (ld["decoded"] == t_out.numpy()[idx].astype(np.float32)).all()
    # values beyond float32's exact range are written as float64, exactly
    assert (ld["comp_size"] == blk.comp_size.numpy().astype(np.float64)).all()
    assert (ld["comp_off"] == blk.comp_off.numpy().astype(np.float64)).all()
    assert (ld["code_lengths"] == blk.code_lengths.numpy().reshape(-1).astype(np.float32)).all()
    assert ld["total"].tolist() == [float(total)] and (ld["decode_errpos"] == -1).all()
