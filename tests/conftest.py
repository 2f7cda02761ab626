import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import __graft_entry__ as entry  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")


def _has_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


def pytest_collection_modifyitems(config, items):
    if _has_gpu():
        return
    skip = pytest.mark.skip(reason="no GPU in this container")
    for it in items:
        if "gpu" in it.keywords:
            it.add_marker(skip)


@pytest.fixture(scope="session")
def orc():
    return entry.load_oracle()


@pytest.fixture(scope="session")
def pkg():
    return entry.load_package()


@pytest.fixture(scope="session")
def vectors():
    with open(os.path.join(GOLDEN, "reference_vectors.json")) as f:
        return json.load(f)


@pytest.fixture(scope="session")
def svc(pkg):
    """One HIP service for the whole GPU session.  Fails loudly (no fallback) if the library is missing."""
    s = pkg.HipCompressionService(chunk_size_mb=1, device=0)
    yield s
    s.close()


def recipe_bytes(orc, recipe):
    """Inputs of tests/golden/reference_vectors.json, by recipe name."""
    if recipe == "AAAABBBBCCCCDDDD":
        return np.frombuffer(b"AAAABBBBCCCCDDDD", dtype=np.uint8)
    if recipe == "A*1024":
        return np.full(1024, 0x41, dtype=np.uint8)
    if recipe == "Hello World! *100":
        return np.frombuffer(("Hello World! " * 100).encode(), dtype=np.uint8)
    if recipe == "Test data for integrity check":
        return np.frombuffer(recipe.encode(), dtype=np.uint8)
    if recipe.startswith("java.util.Random(42).nextBytes("):
        return orc.java_random_bytes(42, int(recipe.split("(")[-1].rstrip(")")))
    if recipe.startswith("i%256"):
        return (np.arange(3 * 1024 * 1024) % 256).astype(np.uint8)
    if recipe.startswith("'A'+(i/100)%26"):
        return (0x41 + (np.arange(512 * 1024) // 100) % 26).astype(np.uint8)
    if recipe.startswith("A*2097152"):
        return np.full(2 * 1024 * 1024, 0x41, dtype=np.uint8)
    raise KeyError(recipe)


def pin_input(orc, pin):
    if "file" in pin:
        return np.fromfile(os.path.join(GOLDEN, pin["file"]), dtype=np.uint8)
    return recipe_bytes(orc, pin["recipe"])


TEXT_TOTAL = 4775113  # cum[96] of the text generator's table (oracle/dcz_oracle.c text_tables)


def text_rank96_positions(seed, start, n):
    """Positions i in [0, n) at which the text generator draws its rarest rank (96), by the generator's own arithmetic."""
    out = []
    with np.errstate(over="ignore"):
        for lo in range(0, n, 1 << 22):
            i = np.arange(lo, min(n, lo + (1 << 22)), dtype=np.uint64)
            x = np.uint64(seed) + (np.uint64(start) + i) * np.uint64(0x9E3779B97F4A7C15)
            x = x + np.uint64(0x9E3779B97F4A7C15)
            x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
            x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
            x = x ^ (x >> np.uint64(31))
            t = ((x >> np.uint64(32)) * np.uint64(TEXT_TOTAL)) >> np.uint64(32)
            out.append(lo + np.nonzero(t == np.uint64(TEXT_TOTAL - 1))[0])
    return np.concatenate(out)
