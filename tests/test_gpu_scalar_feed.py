"""The scalar-fed latency kernel (qsmd5_batch_sf_kernel) through
qsmd5_hash_batch_device_async, which always asks for the 64-lane latency
kernel: QSMD5_PC_FEED=sgpr takes the scalar-fed kernel wherever it is eligible,
QSMD5_PC_FEED=lds keeps the LDS-fed one (the control).  Every digest is
compared with the oracle and, where a chunk is a prefix of the LCG stream of
tests/golden/lcg_lengths.json, with that fixture.

The kernel's boundaries: a phase is 3 blocks (192 B), a workgroup holds 3
chains, the ring has two halves (so 3 phases wrap it), launches above 512
chunks go to the LDS-fed kernel (so n = 513 below runs that one).  The lengths and counts around 8-block
phases and 8-chain workgroups are kept as well.
"""
import ctypes
import random

import numpy as np
import pytest

import qsmd5
from oracle_util import lcg_bytes, md5_many

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

PHASE = 3 * 64
LENS = [0, 1, 55, 56, 63, 64, 65, 119, 120,
        PHASE - 1, PHASE, PHASE + 1, 2 * PHASE, 3 * PHASE + 64,   # 3-block phases
        511, 512, 513, 1024, 17 * 64 + 5, 3 * 512 + 64]           # 8-block phases
COUNTS = [1, 2, 3, 4, 7, 8, 9, 10, 64, 65, 512, 513]
SEED = 12345  # the seed of lcg_lengths.json
POOL = 1 << 16


@pytest.fixture(scope="module")
def pool():
    host = lcg_bytes(SEED, POOL)
    dev = torch.frombuffer(bytearray(bytes(host)), dtype=torch.uint8).cuda()
    return host, dev


@pytest.fixture(scope="module")
def golden_by_len(golden):
    return {c["len"]: bytes.fromhex(c["md5"]) for c in golden("lcg_lengths.json")["cases"]}


def _hash(dev, chunks, order=None, stream=None):
    """chunks: (offset into the pool, length); returns the digests enqueued on `stream`."""
    n = len(chunks)
    desc = torch.tensor([[dev.data_ptr() + o, L] for o, L in chunks], dtype=torch.int64).cuda()
    dig = torch.zeros((n, 16), dtype=torch.uint8, device="cuda")
    od = None
    if order is not None:
        od = torch.tensor(order, dtype=torch.int32).cuda()
    s = stream or torch.cuda.current_stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        qsmd5.hash_device(desc.data_ptr(), dig.data_ptr(), n,
                          order_dev=od.data_ptr() if od is not None else None,
                          stream=s.cuda_stream)
    return dig, (desc, od)


def _want(host, chunks):
    base = ctypes.addressof(host)
    return md5_many([(base + o, L) for o, L in chunks])


def _digests(dig):
    torch.cuda.synchronize()
    return [bytes(r) for r in dig.cpu().numpy()]


@pytest.mark.parametrize("feed", ["sgpr", "lds"])
def test_lengths_and_counts(pool, golden_by_len, monkeypatch, feed):
    monkeypatch.setenv("QSMD5_PC_FEED", feed)
    host, dev = pool
    for n in COUNTS:
        chunks = [(0, LENS[(i + n) % len(LENS)]) for i in range(n)]
        dig, _keep = _hash(dev, chunks)
        got = _digests(dig)
        assert got == _want(host, chunks), "n=%d" % n
        for (_, L), d in zip(chunks, got):
            if L in golden_by_len:
                assert d == golden_by_len[L], "n=%d len=%d" % (n, L)


@pytest.mark.parametrize("feed", ["sgpr", "lds"])
def test_misaligned_pointers(pool, monkeypatch, feed):
    monkeypatch.setenv("QSMD5_PC_FEED", feed)
    host, dev = pool
    chunks = [(16 * i + off, L) for off in range(4) for i, L in enumerate(LENS)]
    dig, _keep = _hash(dev, chunks)
    assert _digests(dig) == _want(host, chunks)


@pytest.mark.parametrize("feed", ["sgpr", "lds"])
def test_ragged_workgroups(pool, monkeypatch, feed):
    """0 to 3 phases (and a block more) inside one workgroup of 3, and of 8."""
    monkeypatch.setenv("QSMD5_PC_FEED", feed)
    host, dev = pool
    lens = [0, 3 * PHASE + 64, PHASE,            # one workgroup of 3
            2 * PHASE + 1, 0, 0,                 # two of its chains idle throughout
            0, 64, 512, 513, 3 * 512, 3 * 512 + 64, 100, 1024]
    chunks = [(3 * i, L) for i, L in enumerate(lens)]
    dig, _keep = _hash(dev, chunks)
    assert _digests(dig) == _want(host, chunks)


@pytest.mark.parametrize("feed", ["sgpr", "lds"])
def test_shuffled_order(pool, monkeypatch, feed):
    monkeypatch.setenv("QSMD5_PC_FEED", feed)
    host, dev = pool
    n = 65
    chunks = [(i, LENS[i % len(LENS)]) for i in range(n)]
    order = list(range(n))
    random.Random(7).shuffle(order)
    dig, _keep = _hash(dev, chunks, order=order)
    assert _digests(dig) == _want(host, chunks)  # digests land by chunk index


def test_two_calls_in_flight(pool, monkeypatch):
    """Two launches on two streams at once: each has ring scratch of its own."""
    monkeypatch.setenv("QSMD5_PC_FEED", "sgpr")
    host, dev = pool
    a = [(0, 40 * PHASE + 7)] * 30
    b = [(1, 40 * PHASE + 70)] * 30
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    da, keep_a = _hash(dev, a, stream=s1)
    db, keep_b = _hash(dev, b, stream=s2)
    assert _digests(da) == _want(host, a)
    assert _digests(db) == _want(host, b)


def test_above_the_chunk_limit_the_lds_fed_kernel_runs(pool, monkeypatch):
    """513 chunks (> 512): the launch goes to the LDS-fed kernel; same digests."""
    monkeypatch.setenv("QSMD5_PC_FEED", "sgpr")
    host, dev = pool
    chunks = [(i % 5, LENS[i % len(LENS)]) for i in range(513)]
    dig, _keep = _hash(dev, chunks)
    assert _digests(dig) == _want(host, chunks)


def test_start_skew_of_long_chunks(monkeypatch):
    """A chunk of >= 32 MiB switches the start skew on for its workgroup: the
    chains start 0, 148 and 40 blocks late (4 x (37 t mod 64)), none on a phase."""
    monkeypatch.setenv("QSMD5_PC_FEED", "sgpr")
    L = (32 << 20) + 5
    t = torch.empty(L, dtype=torch.uint8, device="cuda")
    qsmd5.synth_fill_lcg(t.data_ptr(), L, L, 99, 1, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    host = np.ascontiguousarray(t.cpu().numpy())
    chunks = [(0, L), (7, 1000), (64, 3 * PHASE), (1, 32 << 20)]
    dig, _keep = _hash(t, chunks)
    got = _digests(dig)
    want = md5_many([(host.ctypes.data + o, n) for o, n in chunks])
    assert got == want
