"""GPU parity on the CRC-32C polynomial (a -msse4.2 reference build's SubspaceCRC32,
client/checksum.cc:56-76): a context created with SUBSPACE_CRC_POLY_CASTAGNOLI runs the
same kernels with Castagnoli tables and operators; every result is checked bit for bit
against the oracle's CRC-32C restatement (pinned by tests/golden/crc32c_kat.json)."""
import json
from pathlib import Path

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from subspace_amd import gpu, slots, synth  # noqa: E402
from test_gpu_base_alignment import INIT2, ragged_batch, run_ragged, run_strided, run_uniform, slot_sizes  # noqa: E402
from test_gpu_output_bounds import run_slot_list  # noqa: E402

gpu_test = pytest.mark.gpu  # (per test: the numpy reference's own test below runs without a GPU)
DEV = "cuda"
M32 = 0xFFFFFFFF
KAT = json.loads((Path(__file__).parent / "golden" / "crc32c_kat.json").read_text())["kats"]


@gpu_test
def test_known_answers_on_device(gpu_ctx_c):
    for k in KAT:
        data = bytes.fromhex(k["data_hex"])
        buf = torch.frombuffer(bytearray(data + bytes(16)), dtype=torch.uint8).to(DEV)
        out = torch.zeros(1, dtype=torch.int32, device=DEV)
        gpu_ctx_c.crc32_ragged(buf, torch.zeros(1, dtype=torch.int64, device=DEV),
                               torch.full((1,), len(data), dtype=torch.int64, device=DEV), out, finalize=True)
        torch.cuda.synchronize()
        assert int(out.item()) & M32 == k["checksum"], k["name"]


@gpu_test
@pytest.mark.parametrize("count", [1, 7, 4097])
def test_uniform4k(gpu_ctx_c, oracle, count):
    buf = torch.empty(count * 4096, dtype=torch.uint8, device=DEV)
    gpu.fill_uniform(buf, 4096, 4096, count, seed=0xC32C)
    out = torch.empty(count, dtype=torch.int32, device=DEV)
    gpu_ctx_c.crc32_uniform(buf, 4096, 4096, count, out)
    torch.cuda.synchronize()
    want = oracle.synth_crc_batch(0xC32C, np.full(count, 4096, dtype=np.uint64), castagnoli=True)
    assert np.array_equal(out.cpu().numpy().view(np.uint32), want)


@gpu_test
@pytest.mark.parametrize("align,lead", [(64, 0), (1, 5)])
def test_ragged(gpu_ctx_c, oracle, align, lead):
    rng = np.random.default_rng(align + lead)
    lengths = rng.integers(0, 50000, 1500).astype(np.uint64)
    lengths[::13] = rng.integers(0, 200, len(lengths[::13]))
    lengths[-2:] = [(3 << 20) + 7, 8192 * 5]
    offsets, total = synth.packed_offsets(lengths, align)
    offsets = offsets + np.uint64(lead)
    buf = torch.empty(int(total) + lead + 64, dtype=torch.uint8, device=DEV)
    d_off = torch.from_numpy(offsets.view(np.int64)).to(DEV)
    d_len = torch.from_numpy(lengths.view(np.int64)).to(DEV)
    gpu.fill_ragged(buf, d_off, d_len, seed=0xC32D)
    out = torch.empty(len(lengths), dtype=torch.int32, device=DEV)
    gpu_ctx_c.crc32_ragged(buf, d_off, d_len, out, init=0x12345678)
    torch.cuda.synchronize()
    want = oracle.synth_crc_batch(0xC32D, lengths, init=0x12345678, castagnoli=True)
    assert np.array_equal(out.cpu().numpy().view(np.uint32), want)


@gpu_test
def test_slots_publish_and_verify(gpu_ctx_c, oracle):
    count, cs, ms = 3000, 4, 16
    ps = slots.compute_prefix_size(cs, ms)
    stride = slots.slot_stride(4096, cs, ms)
    rng = np.random.default_rng(3)
    sizes = np.full(count, 4096, dtype=np.uint64)
    host = rng.integers(0, 256, stride * count, dtype=np.uint8)
    host.reshape(count, stride)[:, :ps] = slots.make_prefixes(count, sizes, checksum_size=cs, metadata_size=ms,
                                                              seed=4)
    want = host.copy()
    po = np.arange(count, dtype=np.uint64) * np.uint64(stride)
    oracle.publish_slots(want, po, po + np.uint64(ps), sizes, cs, ms, castagnoli=True)
    dev = torch.from_numpy(host).to(DEV)
    gpu_ctx_c.crc32_slots_strided(dev, stride, count, message_size=4096, checksum_size=cs, metadata_size=ms,
                                  mode=gpu.SLOT_CALCULATE)
    torch.cuda.synchronize()
    assert np.array_equal(dev.cpu().numpy(), want)
    dev[17 * stride + ps + 100] ^= 1
    status = torch.zeros(count, dtype=torch.int32, device=DEV)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    gpu_ctx_c.crc32_slots_strided(dev, stride, count, message_size=4096, checksum_size=cs, metadata_size=ms,
                                  mode=gpu.SLOT_VERIFY, status=status, error_count=err)
    torch.cuda.synchronize()
    assert int(err.item()) == 1 and np.nonzero(status.cpu().numpy())[0].tolist() == [17]


@gpu_test
def test_bad_polynomial_rejected():
    with pytest.raises(gpu.CrcError):
        gpu.CrcContext(0, poly=0x04C11DB7)  # non-reflected form: no x^0 term in bit 31


# ------------------------------------------------------------------ every other kernel on CRC-32C
# The paths above are three of a dozen. Each operator family is built per polynomial in
# subspace_crc_ctx_create_poly (the small kernel's padding inverses and Z_C, pow2, the nibble
# inverses): a table slot filled from the wrong source, or a constant left in a kernel, passes
# every IEEE test. Inputs are numpy-random bytes; the oracle's CRC-32C over the host copy is
# the reference.

def crc32c_batch(oracle):
    """oracle.crc32_batch's signature on the Castagnoli polynomial (the SSE4.2 batch where the
    CPU has it, else one oracle.crc32c per message)."""
    def batch(host, offsets, lengths, init=M32):
        if oracle.has_sse42():
            return oracle.crc32c_sse42_batch(host, offsets, lengths, init)
        return np.array([oracle.crc32c(init, host[int(o):int(o) + int(n)].tobytes())
                         for o, n in zip(offsets, lengths)], dtype=np.uint32)
    return batch


@gpu_test
@pytest.mark.parametrize("length", [64, 200, 1000, 2048, 4081])
def test_uniform_small_16b_strides(gpu_ctx_c, oracle, length):
    """The small kernel's uniform FAST form, G = 1 .. 32 lanes per message."""
    run_uniform(gpu_ctx_c, oracle, length, (length + 15) & ~15, 301, 0, seed=length, crc_batch=crc32c_batch(oracle))


@gpu_test
def test_uniform_small_packed_stride(gpu_ctx_c, oracle):
    run_uniform(gpu_ctx_c, oracle, 777, 781, 301, 0, seed=777, crc_batch=crc32c_batch(oracle))


@gpu_test
def test_uniform_long(gpu_ctx_c, oracle):
    """crc32_long_kernel, the segment scans and crc32_long_final_kernel."""
    run_uniform(gpu_ctx_c, oracle, 16384, 16384, 37, 0, seed=16384, crc_batch=crc32c_batch(oracle))


@gpu_test
@pytest.mark.parametrize("k", [15])
def test_uniform_misaligned_base(gpu_ctx_c, oracle, k):
    run_uniform(gpu_ctx_c, oracle, 1000, 1008, 301, k, seed=1015, crc_batch=crc32c_batch(oracle))


@gpu_test
@pytest.mark.parametrize("k", [15])
def test_ragged_misaligned_base(gpu_ctx_c, oracle, k):
    b = ragged_batch()
    want = crc32c_batch(oracle)(b["host"], b["offsets"] + np.uint64(k), b["lengths"], INIT2) ^ np.uint32(M32)
    run_ragged(gpu_ctx_c, k, 1, True, want)


# (slot size, max_message_size, metadata_size, payload sizes from .. to, count)
SLOT_LISTS_C = {
    "4k-full": (4096, 4096, 0, 4096, 4096, 2001),     # FAST waves
    "4k-short": (4096, 4096, 0, 0, 500, 2001),        # the waves repack (REPACK2)
    "256": (256, 256, 0, 0, 256, 2001),               # packed form, G = 2
    "4k-meta100": (4096, 4096, 100, 0, 4096, 2001),   # small kernel + crc32_slot_finish_kernel (pow2)
    "32k": (32768, 32768, 0, 1, 32767, 1501),         # ragged pipeline at absolute addresses + slot finish
}


@gpu_test
@pytest.mark.parametrize("name", list(SLOT_LISTS_C))
def test_slot_lists(gpu_ctx_c, oracle, name):
    slot_size, bound, ms, lo, hi, count = SLOT_LISTS_C[name]
    sizes = np.random.default_rng(hi + ms).integers(lo, hi + 1, count).astype(np.uint64)
    run_slot_list(gpu_ctx_c, oracle, count, slot_size, bound, 4, ms, sizes, seed=bound + ms + lo, castagnoli=True)


@gpu_test
def test_slot_list_longer_than_bound(gpu_ctx_c, oracle):
    """Messages longer than max_message_size (every 40th, up to 9,000 B against a bound of 256):
    the small kernel's long-message flush -- 8 KiB chunks joined by Z_8192, the last chunk's
    padding undone with the inverses up to Z_4096^{-1}, the slot finished as Z_L(H) ^ crc."""
    count = 2001
    rng = np.random.default_rng(9000)
    sizes = rng.integers(0, 257, count).astype(np.uint64)
    sizes[::40] = rng.integers(257, 9001, len(sizes[::40]))
    sizes[:3] = [9000, 8192, 4097]
    run_slot_list(gpu_ctx_c, oracle, count, 9000, 256, 4, 0, sizes, seed=9001, castagnoli=True)


@gpu_test
def test_strided_per_slot_sizes(gpu_ctx_c, oracle):
    run_strided(gpu_ctx_c, oracle, 2001, 1000, 4, 0, slot_sizes(2001, 1000, 5), 0, seed=1000, castagnoli=True)


# ------------------------------------------------------------------ a third polynomial
POLY_BASE91_D = 0xD419CC15  # CRC-32/BASE91-D, reflected; check value 0x87315576


def crc_table(poly):
    t = np.arange(256, dtype=np.uint32)
    for _ in range(8):
        t = np.where(t & 1, (t >> 1) ^ np.uint32(poly), t >> 1).astype(np.uint32)
    return t


def crc_np(poly, init, rows, lengths=None):
    """Raw-state reflected CRC of every row of `rows` ((n, L) uint8), byte by byte over the
    256-entry table, all rows at once; lengths: per-row byte counts (rows zero-padded)."""
    tab = crc_table(poly)
    rows = np.asarray(rows, dtype=np.uint8)
    crc = np.full(rows.shape[0], init & M32, dtype=np.uint32)
    for j in range(rows.shape[1]):
        nxt = tab[(crc ^ rows[:, j]) & np.uint32(0xFF)] ^ (crc >> np.uint32(8))
        crc = nxt if lengths is None else np.where(j < lengths, nxt, crc)
    return crc


def test_numpy_reference(oracle):
    """crc_np against the oracle on both named polynomials (random data, random inits, ragged
    rows) and against the three catalogued check values over b"123456789"."""
    check = np.frombuffer(b"123456789", dtype=np.uint8)[None, :]
    for poly, value in ((gpu.POLY_IEEE, 0xCBF43926), (gpu.POLY_CASTAGNOLI, 0xE3069283), (POLY_BASE91_D, 0x87315576)):
        assert int(crc_np(poly, M32, check)[0]) ^ M32 == value
    rng = np.random.default_rng(91)
    rows = rng.integers(0, 256, (40, 700), dtype=np.uint8)
    lengths = rng.integers(0, 701, 40)
    lengths[:3] = [0, 1, 700]
    for init in (M32, 0, 0x12345678):
        for poly, ref in ((gpu.POLY_IEEE, oracle.crc32), (gpu.POLY_CASTAGNOLI, oracle.crc32c)):
            assert crc_np(poly, init, rows).tolist() == [ref(init, r.tobytes()) for r in rows]
            assert crc_np(poly, init, rows, lengths).tolist() == [ref(init, r[:n].tobytes())
                                                                  for r, n in zip(rows, lengths)]


@gpu_test
@pytest.mark.parametrize("length,stride,count", [(4096, 4096, 65), (200, 208, 301), (16384, 16384, 5)])
def test_third_polynomial_uniform(length, stride, count):
    """The 4 KiB kernel, the small kernel and the long kernel on a polynomial that is neither of
    the named ones: a context's tables and operators come from its polynomial alone."""
    rng = np.random.default_rng(length)
    host = rng.integers(0, 256, count * stride + 64, dtype=np.uint8)
    dev = torch.from_numpy(host).to(DEV)
    out = torch.full((count,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    with gpu.CrcContext(0, poly=POLY_BASE91_D) as ctx:
        ctx.crc32_uniform(dev, stride, length, count, out, init=INIT2, finalize=True)
        torch.cuda.synchronize()
    want = crc_np(POLY_BASE91_D, INIT2, host[:count * stride].reshape(count, stride)[:, :length]) ^ np.uint32(M32)
    assert np.array_equal(out.cpu().numpy().view(np.uint32), want)


@gpu_test
def test_third_polynomial_ragged():
    rng = np.random.default_rng(64)
    lengths = rng.integers(0, 20001, 64).astype(np.uint64)
    lengths[:4] = [0, 1, 8192, 20000]
    offs, total = synth.packed_offsets(lengths, 1)
    offs = offs + np.uint64(7)
    host = rng.integers(0, 256, int(total) + 7 + 64, dtype=np.uint8)
    rows = np.zeros((64, 20000), dtype=np.uint8)
    for i, (o, n) in enumerate(zip(offs, lengths)):
        rows[i, :int(n)] = host[int(o):int(o) + int(n)]
    dev = torch.from_numpy(host).to(DEV)
    out = torch.full((64,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    with gpu.CrcContext(0, poly=POLY_BASE91_D) as ctx:
        ctx.crc32_ragged(dev, torch.from_numpy(offs.view(np.int64)).to(DEV),
                         torch.from_numpy(lengths.view(np.int64)).to(DEV), out)
        torch.cuda.synchronize()
    want = crc_np(POLY_BASE91_D, M32, rows, lengths.astype(np.int64))
    assert np.array_equal(out.cpu().numpy().view(np.uint32), want)
