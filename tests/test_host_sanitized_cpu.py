"""The host-only pieces of the detect path under AddressSanitizer + UBSan ("the build should add its own"; VERDICT r2
missing #5): csrc/opd_loader.cpp (the safetensors parser that reads an untrusted file) and csrc/opd_host.cpp (Pillow coefficient
tables, mask down-sampling, sine position embedding, person filter + NMS) are compiled with g++ -fsanitize=address,undefined together
with tests/native/host_asan_driver.cpp and run on the CPU over well-formed, schema-violating, truncated and bit-flipped checkpoints.
Any sanitizer report fails the test.  (GPU code is never run under a sanitizer: the pool refuses it.)"""

import json
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from office_person_detection_vit_amd.weights import DetrArch, save_safetensors, synth_weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "office_person_detection_vit_amd", "csrc")


def _rewrite_header(src, dst, edit):
    """Copy a safetensors file with its JSON header passed through ``edit`` (the data section is untouched)."""
    with open(src, "rb") as f:
        n = struct.unpack("<Q", f.read(8))[0]
        header = json.loads(f.read(n))
        data = f.read()
    header = edit(header)
    h = json.dumps(header, separators=(",", ":")).encode()
    with open(dst, "wb") as f:
        f.write(struct.pack("<Q", len(h)) + h + data)


# ---- the weight packers of csrc/opd_pack.cpp, restated in numpy from their layout comments (never from the C++) ----------------------------

def _expect_permute_k32(w):
    """Within each 32-block of K: slot 8g+e <- channel 4g+e, slot 8g+4+e <- channel 16+4g+e."""
    rows, K = w.shape
    return w.reshape(rows, K // 32, 2, 4, 4).transpose(0, 1, 3, 2, 4).reshape(rows, K)   # [n][block][half][g][e] -> [n][block][g][half][e]


def _frag(tile, ks):
    """One 1 KiB piece: lane L = 16 g + li holds tile[li][32 ks + 8 g .. + 7] (tile: 16 rows)."""
    return np.ascontiguousarray(tile[:, 32 * ks:32 * ks + 32].reshape(16, 4, 8).transpose(1, 0, 2))


def _split_values(N, K):
    """fp32 inputs of opd_split_f16_frag: the edges of `hi` (signed zeros, 2^-14 and its fp32 neighbours, fp16 subnormal steps, the fp16
    maximum), fp16-exact values, values whose `lo` lies exactly between two fp16 numbers (both parities), then weights-like random values."""
    rng = np.random.default_rng(N * 1000 + K)
    t = np.float32(2.0 ** -14)
    edge = [0.0, t, np.nextafter(t, np.float32(0)), np.nextafter(t, np.float32(1)), 2.0 ** -24, 2.0 ** -25, 65504.0, 60000.0, 1.0, 0.333251953125]
    ties = []
    for h in (2.0 ** -4, 0.09375, 2.0 ** -9 * 1.5):          # fp16-exact hi with room below its half ulp for a 12-bit lo
        ulp = 2.0 ** (np.floor(np.log2(h)) - 10)
        for m in (2049, 2051, 4093):                          # lo = m * 2^e with a 12-bit odd m: a tie between two 11-bit neighbours
            e = np.floor(np.log2(ulp / 2 * 2048 / m))        # the largest lo with (v - h) below half an fp16 ulp of h
            v = h + m * 2.0 ** e / 2048
            assert float(np.float32(v)) == v and float(np.float16(np.float32(v))) == h, (h, m)   # exact in fp32, and hi is h
            ties.append(v)
    special = np.asarray(edge + ties, np.float32)
    special = np.concatenate([special, -special])
    exact = rng.standard_normal(24).astype(np.float16).astype(np.float32)
    w = (rng.standard_normal(N * K) * 0.05).astype(np.float32)
    w[:special.size] = special
    w[special.size:special.size + exact.size] = exact
    return rng.permutation(w).reshape(N, K)


def _expect_split_f16_frag(w):
    """Per (16-row tile, 32-wide k-step): 1 KiB of hi, then 1 KiB of lo, each in fragment order; hi = 0 where |v| < 2^-14, else float16(v);
    lo = float16((v - hi) * 2048)."""
    N, K = w.shape
    hi = np.where(np.abs(w) < np.float32(2.0 ** -14), np.float16(0), w.astype(np.float16))
    with np.errstate(over="ignore"):
        lo = ((w - hi.astype(np.float32)) * np.float32(2048)).astype(np.float16)
    return np.stack([np.stack([np.stack([_frag(m[16 * nt:16 * nt + 16], ks) for m in (hi, lo)]) for ks in range(K // 32)]) for nt in range(N // 16)])


def _expect_encffn_pack(w1, b1, w2, wt, bt, tail, wo):
    """The eight per-wave streams of enc_ffn_kernel: [front] G0(0) G1(0) G0(1) { G1(c+1) G2(c) G3(c) G0(c+2) } [tail passes, five zero pieces]."""
    nch = w1.shape[0] // 128
    b = lambda a: np.ascontiguousarray(a).view(np.uint8).ravel()
    zero = lambda n: np.zeros(n * 1024, np.uint8)
    lanes_g, lanes_li = np.arange(64) >> 4, np.arange(64) & 15
    out = []
    for w in range(8):
        def fc2_group(mat, row0, col0, i0):   # pieces 2 i + j: k-step i0 + i of the wave's 16-row tiles j = 0, 1
            return [b(_frag(mat[row0 + (2 * w + j) * 16:row0 + (2 * w + j) * 16 + 16, col0:], i0 + i)) for i in range(2) for j in range(2)]

        def g0(c):   # the bias piece (lane (g, li): b1[128 c + 16 w + 4 g .. + 3]), then k-steps 0 .. 3 of W1's tile
            if c >= nch:
                return [zero(5)]
            bias = np.stack([b1[128 * c + 16 * w + 4 * g:128 * c + 16 * w + 4 * g + 4] for g in lanes_g])
            return [b(bias)] + [b(_frag(w1[128 * c + 16 * w:128 * c + 16 * w + 16], ks)) for ks in range(4)]

        def g1(c):
            return [zero(4)] if c >= nch else [b(_frag(w1[128 * c + 16 * w:128 * c + 16 * w + 16], ks)) for ks in range(4, 8)]

        s = []
        if wo is not None:
            for q in range(4):
                s += fc2_group(wo, 0, 0, 2 * q)
        s += g0(0) + g1(0) + g0(1)
        for c in range(nch):
            s += g1(c + 1) + fc2_group(w2, 0, 128 * c, 0) + fc2_group(w2, 0, 128 * c, 2) + g0(c + 2)
        for t in range(tail):
            s.append(b(np.stack([bt[256 * t + (2 * w + (li >> 3)) * 16 + 4 * g:][:4] for g, li in zip(lanes_g, lanes_li)])))
            for q in range(4):
                s += fc2_group(wt, 256 * t, 0, 2 * q)
        if tail:
            s.append(zero(5))
        out.append(np.concatenate(s))
    assert len({o.size for o in out}) == 1
    return np.concatenate(out)


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++ for the sanitizer build")
def test_host_code_under_address_and_ub_sanitizers(tmp_path):
    exe = str(tmp_path / "host_asan_driver")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
           os.path.join(ROOT, "tests", "native", "host_asan_driver.cpp"), os.path.join(CSRC, "opd_loader.cpp"), os.path.join(CSRC, "opd_host.cpp"),
           os.path.join(CSRC, "opd_pack.cpp"), "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    split_in = {(N, K): _split_values(N, K) for N, K in ((16, 32), (32, 64))}
    for (N, K), w in split_in.items():
        w.tofile(str(tmp_path / f"pack_split_{N}x{K}.in"))

    files, expect = [], {}
    # (1) a real (shallow) architecture: well-formed, then header edits that violate the schema
    arch = DetrArch(depths=(1, 1, 1, 1), encoder_layers=1, decoder_layers=1, num_queries=7)
    good = str(tmp_path / "good.safetensors")
    save_safetensors(synth_weights(arch, 3, 1.0, calibrate=False), good)
    expect["good.safetensors"] = (0, 0)

    def drop(key):
        return lambda h: {k: v for k, v in h.items() if k != key}

    def reshape(key, shape):
        def f(h):
            h = dict(h)
            h[key] = dict(h[key], shape=shape)
            return h
        return f

    def dtype(key, dt):
        def f(h):
            h = dict(h)
            h[key] = dict(h[key], dtype=dt)
            return h
        return f

    def offsets(key, off):
        def f(h):
            h = dict(h)
            h[key] = dict(h[key], data_offsets=off)
            return h
        return f
    k_w = "model.input_projection.weight"
    edits = {
        "missing_tensor": (drop("model.decoder.layers.0.encoder_attn.k_proj.bias"), (0, -3)),
        "wrong_shape": (reshape(k_w, [256, 1024, 2, 1]), (0, -3)),
        "shape_overflow": (reshape(k_w, [2 ** 40, 2 ** 40, 2 ** 40, 1]), None),
        "negative_dim": (reshape(k_w, [-256, 2048, 1, 1]), None),
        "empty_shape": (reshape(k_w, []), None),
        "unknown_dtype": (dtype(k_w, "F8_E4M3"), None),
        "offsets_reversed": (offsets(k_w, [10 ** 9, 4]), None),
        "offsets_past_eof": (offsets(k_w, [0, 2 ** 62]), None),
        "offsets_negative": (offsets(k_w, [-8, 8]), None),
        "offsets_not_a_list": (offsets(k_w, "0:8"), None),
    }
    for name, (edit, exp) in edits.items():
        p = str(tmp_path / f"{name}.safetensors")
        _rewrite_header(good, p, edit)
        files.append(p)
        if exp is not None:
            expect[os.path.basename(p)] = exp
    files.insert(0, good)
    files.append(str(tmp_path / "does_not_exist.safetensors"))
    # (2) a small file: truncations at every interesting length, bit flips in the header, absurd header lengths
    small = str(tmp_path / "small.safetensors")
    save_safetensors({"a": np.arange(12, dtype=np.float32).reshape(3, 4), "b.weight": np.ones((2, 2), np.float32),
                      "c": np.zeros((5,), np.float32)}, small)
    raw = open(small, "rb").read()
    hlen = struct.unpack("<Q", raw[:8])[0]
    rng = np.random.default_rng(0)
    cuts = sorted(set([0, 1, 7, 8, 9, 8 + hlen - 1, 8 + hlen, 8 + hlen + 1, len(raw) - 1] + [int(x) for x in rng.integers(0, len(raw), 40)]))
    for c in cuts:
        p = str(tmp_path / f"cut_{c}.safetensors")
        open(p, "wb").write(raw[:c])
        files.append(p)
    for i in range(150):
        b = bytearray(raw)
        for _ in range(int(rng.integers(1, 4))):
            pos = int(rng.integers(0, 8 + hlen))
            b[pos] ^= 1 << int(rng.integers(0, 8))
        p = str(tmp_path / f"flip_{i}.safetensors")
        open(p, "wb").write(bytes(b))
        files.append(p)
    for i, n in enumerate((0, 1, 2 ** 31, 2 ** 63, 2 ** 64 - 1, len(raw), len(raw) - 8)):
        p = str(tmp_path / f"hlen_{i}.safetensors")
        open(p, "wb").write(struct.pack("<Q", n) + raw[8:])
        files.append(p)
    lst = str(tmp_path / "files.txt")
    open(lst, "w").write("\n".join(files) + "\n")

    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:allocator_may_return_null=1", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([exe, lst], capture_output=True, text=True, env=env, timeout=600)
    assert "Sanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-4000:]
    assert run.returncode == 0, (run.returncode, run.stdout[-2000:], run.stderr[-4000:])
    seen = {}
    for line in run.stdout.splitlines():
        if line.startswith("file "):
            w = line.split()
            seen[w[1]] = (int(w[3]), int(w[5]))
    assert len(seen) == len(files)
    for name, exp in expect.items():
        assert seen[name] == exp, (name, seen[name], exp)
    assert seen["does_not_exist.safetensors"][0] == -2
    for name, (parse, schema) in seen.items():      # every malformed file is REFUSED with an error code, never accepted by accident
        if name.startswith(("cut_", "hlen_")) and name not in ("hlen_5.safetensors",):
            assert parse != 0 or schema != 0, name
    assert "nms kept" in run.stdout and "position embedding sum" in run.stdout
    # the weight packers: the bytes the driver wrote against numpy restatements of the layout comments in csrc/opd_pack.cpp
    packed = lambda name, dt: np.fromfile(str(tmp_path / name), dt)
    for K in (32, 96):
        assert np.array_equal(packed(f"pack_permute_K{K}.bin", np.uint16), _expect_permute_k32(np.arange(3 * K, dtype=np.uint16).reshape(3, K)).ravel()), K
    for (N, K), w in split_in.items():
        got, exp = packed(f"pack_split_{N}x{K}.bin", np.uint16), _expect_split_f16_frag(w).view(np.uint16).ravel()
        assert got.size == 2 * N * K and np.array_equal(got, exp), (N, K, np.flatnonzero(got != exp)[:8])
    for F, tail, front in ((128, 0, False), (256, 2, True)):
        # distinct inside every run of 65536 elements, run r shifted by 0x1235 r: the two tail passes of Wt differ at every (row, column)
        ids = lambda n, mul, add: ((np.arange(n, dtype=np.uint64) * mul + add + (np.arange(n, dtype=np.uint64) >> 16) * 0x1235) & 0xffff).astype(np.uint16)
        exp = _expect_encffn_pack(ids(F * 256, 1, 0).reshape(F, 256), 1000 + np.arange(F, dtype=np.float32), ids(256 * F, 3, 1).reshape(256, F),
                                  ids(tail * 65536, 5, 2).reshape(tail * 256, 256), 5000 + np.arange(tail * 256, dtype=np.float32), tail,
                                  ids(65536, 7, 3).reshape(256, 256) if front else None)
        got = packed(f"pack_encffn_F{F}.bin", np.uint8)
        pieces = (16 if front else 0) + 14 + 17 * (F // 128) + (17 * tail + 5 if tail else 0)   # per wave: opd_pack.h
        assert got.size == exp.size == 8 * pieces * 1024, (F, got.size, exp.size)   # = opd_encffn_pack_bytes: the driver allocated and wrote that many
        assert f"pack pack_encffn_F{F}.bin bytes {8 * pieces * 1024}\n" in run.stdout
        assert np.array_equal(got, exp), (F, np.flatnonzero(got != exp)[:8])
