"""The whole forward at the architectures the loader accepts besides the 6 + 6 layer, 100-query, 92-row model every other end-to-end
test runs: one layer each side, the query / class maxima and minima, a query count the fused decoder does not take, and the decoder depths
on either side of where the memory K/V projection no longer fits the encoder's last launch (OPD_ENC_TAIL=1 handles).  Each against the oracle run live on the same seeded
weights (depths (1, 1, 1, 1), attention gain 1.0) and frames, at the bounds of tests/test_detector_gpu.py for these weights and this frame
size (TOL[1.0]: the 6 + 6 model's bound; shallower models accumulate less error, so nothing new is introduced).

Every handle here is created in poison mode (0xFF in every buffer, red zones around each): a kernel that reads workspace it has not
written shows as NaN, one that writes next to a buffer sized by the architecture shows in the red-zone scan."""

import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from office_person_detection_vit_amd import HipDetrDetector, _capi
from office_person_detection_vit_amd.frames import structured_frames
from office_person_detection_vit_amd.weights import DetrArch, ensure_weight_file, load_safetensors
from oracle import detr_oracle as O

from arch_common import DET, compare_records
from plan_common import FFN_ONE_LAUNCH, HEADS_SPLIT16, QKV_LAUNCH, transformer_plan

pytestmark = pytest.mark.gpu

TOL_BOX, TOL_PROB, TOL_ENC = 2e-3, 4e-3, 3e-2   # tests/test_detector_gpu.py::TOL[1.0]
H, W = 256, 320

#        id            enc dec queries labels
ARCHS = {"one_layer": (1, 1, 100, 91),    # first = last encoder layer; fused decoder with layer 0 only (no dec_qkv / dec_self)
         "max_q_cls": (2, 2, 128, 127),   # no key padding, full class tiles, full post-process block
         "min_q_cls": (1, 2, 4, 2),       # (two labels: the seeded weights favour class 1, which must not be the no-object row)
         "chain_q50": (1, 2, 50, 91),     # Q & 3 != 0: the chain decoder
         "tail16": (1, 8, 20, 91),        # 16 tail passes, the most enc_ffn_kernel takes
         "kv_launch": (1, 9, 20, 91)}     # 2 * dec_layers > 16: the memory K/V projection as its own launch
# OPD_ENC_TAIL=1 (off by default): every encoder FFN launch also projects what consumes its output, the next layer's q | k | v or, behind the
# last layer, the decoder's memory K/V as 2 * dec_layers tail passes while that is <= 16 (csrc/opd_weights.cpp::build_encoder_ffn_packs)
TAIL = "+enc_tail"
TAIL_KEYS = [k + TAIL for k in ("one_layer", "max_q_cls", "tail16", "kv_launch")]


def _arch(key):
    e, d, q, l = ARCHS[key.replace(TAIL, "")]
    return DetrArch(depths=(1, 1, 1, 1), encoder_layers=e, decoder_layers=d, num_queries=q, num_labels=l)


def _softmax(x):
    return torch.softmax(torch.from_numpy(np.asarray(x)), -1).numpy()


def _poisoned(path, **kw):
    lib = _capi.load_library()
    lib.opd_test_set_alloc_poison(0xFF)
    try:
        det = HipDetrDetector(model_path=path, **kw)
        det.load_model()
    finally:
        lib.opd_test_set_alloc_poison(-1)
    return det


def _redzones_intact(det):
    bad = _capi.load_library().opd_test_check_redzones(C.c_void_p(det.model))
    assert bad == 0, f"{bad} buffers with a damaged red zone; first: {_capi.last_error()}"


class Ctx:
    """One architecture: its weight file (own tag: the cache file name does not encode the architecture), ONE handle for the module, the
    oracle's outputs and the handle's raw outputs on the two test frames, each computed once."""

    def __init__(self, key, cache):
        self.key = key
        self.path = ensure_weight_file(cache, _arch(key), 0, 1.0, "arch_" + key.replace(TAIL, ""))
        self.frames = structured_frames(2, H, W, seed=999)
        # (a handle of the deployed kind: configured for more than ~1400 tokens, so that the encoder runs its row-owner launches, whose last
        #  one can carry the decoder's memory K/V as tail passes; smaller handles run split-K GEMMs instead)
        if key.endswith(TAIL):
            os.environ["OPD_ENC_TAIL"] = "1"   # (read once, when the handle is created)
        try:
            self.det = _poisoned(self.path, confidence_threshold=0.5, max_batch=8, max_size=(480, 640), resize=False)
        finally:
            os.environ.pop("OPD_ENC_TAIL", None)
        pv, pm = O.preprocess(self.frames)
        lg, bx, mem = O.forward(O.to_torch(load_safetensors(self.path)), pv, pm)
        self.oracle = (lg.numpy(), bx.numpy(), mem.numpy())
        self.raw = self.det.forward_raw(self.frames)

    def kernel_table(self):
        """{kernel name: launches} of one eagerly launched, profiled forward."""
        lib = _capi.load_library()
        self.det.set_profiling(True)
        try:
            self.det.forward_raw(self.frames)
            rows = (_capi.OpdKernelStat * 256)()
            n = C.c_int()
            _capi.check(lib.opd_detr_kernel_table(C.c_void_p(self.det.model), rows, 256, C.byref(n)), "opd_detr_kernel_table")
            return {rows[i].name.decode(): int(rows[i].launches) for i in range(min(n.value, 256))}
        finally:
            self.det.set_profiling(False)


@pytest.fixture(scope="module")
def ctx(weight_cache):
    made = {}

    def get(key):
        if key not in made:
            made[key] = Ctx(key, weight_cache)
        return made[key]

    yield get
    for c in made.values():
        c.det.close()


@pytest.mark.parametrize("key", list(ARCHS) + TAIL_KEYS)
def test_forward_matches_live_oracle(ctx, parity_log, key):
    c = ctx(key)
    e, d, q, l = ARCHS[key.replace(TAIL, "")]
    (lg0, bx0, mem0), (logits, boxes, enc) = c.oracle, c.raw
    assert logits.shape == (2, q, l + 1) and boxes.shape == (2, q, 4) and enc.shape == mem0.shape
    assert np.isfinite(logits).all() and np.isfinite(boxes).all() and np.isfinite(enc).all()
    dbox = float(np.abs(boxes - bx0).max())
    dprob = float(np.abs(_softmax(logits) - _softmax(lg0)).max())
    denc = float(np.abs(enc - mem0).max())
    parity_log(f"arch {key} ({e}+{d} layers, {q} queries, {l + 1} rows) {H}x{W} vs live oracle", dbox, dprob, denc, TOL_BOX)
    print(f"arch {key}: |dbox| {dbox:.3e} |dprob| {dprob:.3e} |denc| {denc:.3e}")
    assert dbox <= TOL_BOX and dprob <= TOL_PROB and denc <= TOL_ENC, (dbox, dprob, denc)
    # the outputs say something: queries are not collapsed; where the ORACLE is confident of a class (four of the six architectures:
    # one_layer peaks at 0.49 and chain_q50 at 0.36 on these frames), so is the device
    assert float(bx0.std(axis=1).mean()) > 5e-3 and float(boxes.std(axis=1).mean()) > 5e-3
    if float(_softmax(lg0)[..., :-1].max()) > 0.5 + TOL_PROB:
        assert float(_softmax(logits)[..., :-1].max()) > 0.5
    else:
        assert key.replace(TAIL, "") in ("one_layer", "chain_q50")
    _redzones_intact(c.det)


def _dec(table, name):
    return table.get(name, 0)


@pytest.mark.parametrize("key", list(ARCHS))
def test_decoder_route_of_each_architecture(ctx, key):
    """Which decoder an architecture gets (the kernel table of a profiled forward): a query count that is no multiple of 4 runs the chain of
    single-fp16-operand launches, the lower-precision route; every other one the fused decoder, whose layer 0 has no dec_qkv / dec_self."""
    e, d, q, l = ARCHS[key]
    table = ctx(key).kernel_table()
    print(f"arch {key}: " + ", ".join(f"{k} x{v}" for k, v in table.items()))
    dec = {k: v for k, v in table.items() if re.match(r"dec_\w+_kernel", k)}
    if key == "chain_q50":
        assert not dec, dec
        return
    assert _dec(table, "dec_cross_out_kernel") == d and _dec(table, "dec_ffn_kernel") == d, table
    assert sum(v for k, v in table.items() if k.startswith("dec_qkv_kernel")) == d - 1, table
    assert _dec(table, "dec_self_kernel") == d - 1, table
    if key == "one_layer":
        assert not any("dec_qkv" in k or "dec_self" in k for k in table), table
    assert any(k.startswith("heads2_kernel") for k in table) and not any(k.startswith("heads_kernel") for k in table), table


def _outside_decoder(table):
    return {k: v for k, v in table.items() if not re.match(r"dec_\w+_kernel", k) and "attention" not in k}


def _launch_difference(a, b):
    return {k: v for k, v in ((k, b.get(k, 0) - a.get(k, 0)) for k in set(a) | set(b)) if v}


def test_memory_kv_leaves_the_encoder_launch_above_eight_decoder_layers(ctx):
    """With the encoder's tail projections on, the last FFN launch projects the decoder's memory keys / values up to 8 decoder layers
    (2 x 8 = 16 passes, the most it takes); from 9 on they are one GEMM launch of their own: between the two architectures the launches
    outside the decoder layers differ by exactly that one.  By default the projection is a launch of its own at every depth, and a second
    encoder layer's q | k | v likewise."""
    outside = {}
    for key in ("tail16", "kv_launch", "tail16" + TAIL, "kv_launch" + TAIL, "max_q_cls", "max_q_cls" + TAIL):
        e, d = ARCHS[key.replace(TAIL, "")][:2]
        table = ctx(key).kernel_table()
        print(f"arch {key}: " + ", ".join(f"{k} x{v}" for k, v in table.items()))
        outside[key] = _outside_decoder(table)
        assert sum(v for k, v in table.items() if "attention" in k) == e + d, table
        assert sum(v for k, v in table.items() if k.startswith("enc_ffn_kernel")) == e, table
    diff = _launch_difference(outside["tail16" + TAIL], outside["kv_launch" + TAIL])
    assert list(diff.values()) == [1] and next(iter(diff)).startswith("conv_gemm"), diff
    assert _launch_difference(outside["tail16"], outside["kv_launch"]) == {}
    assert _launch_difference(outside["kv_launch" + TAIL], outside["kv_launch"]) == {}
    # 2 encoder + 2 decoder layers: the tails save the second layer's q | k | v launch and the memory K/V launch
    diff = _launch_difference(outside["max_q_cls"], outside["max_q_cls" + TAIL])
    assert list(diff.values()) == [-2] and next(iter(diff)).startswith("conv_gemm"), diff


def test_transformer_plan_agrees_with_the_kernel_table(ctx):
    """plan_transformer, asked through its CPU hook for each handle's architecture, bounds and environment, names the launches that handle's
    profiled forward ran: the one-launch encoder FFNs, the fused decoder's kernels (none for the chain), the heads kernel, and -- as the
    count of implicit-GEMM launches beyond the trunk's, which every handle here shares -- each layer's own q | k | v projection and the
    memory K/V projection."""
    beyond_plan = {}
    for key in list(ARCHS) + TAIL_KEYS:
        e, d, q, l = ARCHS[key.replace(TAIL, "")]
        head, enc = transformer_plan((e, d, q, l + 1), (480, 640, 8), 2, H, W, {"OPD_ENC_TAIL": "1"} if key.endswith(TAIL) else None)
        table = ctx(key).kernel_table()
        count = lambda prefix: sum(v for k, v in table.items() if k.startswith(prefix))
        assert count("enc_ffn_kernel") == sum(step[2] == FFN_ONE_LAUNCH for step in enc), (key, table)
        fused = {"dec_qkv_kernel": d - 1, "dec_self_kernel": d - 1, "dec_cross_out_kernel": d, "dec_ffn_kernel": d}
        assert {k: count(k) for k in fused} == (fused if head["dec_fused"] else dict.fromkeys(fused, 0)), (key, table)
        assert not {k for k in table if re.match(r"dec_\w+_kernel", k) and not k.startswith(tuple(fused))}, (key, table)
        assert (count("heads2_kernel"), count("heads_kernel")) == ((1, 0) if head["heads"] == HEADS_SPLIT16 else (0, 1)), (key, table)
        assert head["dec_fused"] or head["dec_small_m"]   # (the chain's linears here are gemm_k256 launches: none of them counts below)
        beyond_plan[key] = count("conv_gemm") - sum(step[0] == QKV_LAUNCH for step in enc) - head["kv_launch"]
    assert len(set(beyond_plan.values())) == 1, beyond_plan


@pytest.mark.parametrize("key", list(ARCHS))
def test_frame_alone_equals_frame_in_batch(ctx, key):
    c = ctx(key)
    logits, boxes, _ = c.raw
    lg1, bx1, _ = c.det.forward_raw([c.frames[1]], want_encoder=False)
    np.testing.assert_allclose(bx1[0], boxes[1], atol=1e-6)   # same kernels, same order: bitwise in practice
    np.testing.assert_allclose(lg1[0], logits[1], atol=1e-6)
    _redzones_intact(c.det)


def _thresholds(scores):
    """Score thresholds that sit in a gap of the ORACLE's scores, at least 1e-2 from the nearest one (the device's probabilities are
    within 4e-3 of the oracle's): the midpoints of the three widest gaps that are wide enough, the ends of [0, 1] included (below every score:
    every query is kept)."""
    s = np.concatenate([[0.0], np.sort(np.asarray(scores, np.float64).ravel()), [1.0]])
    gaps = np.diff(s)
    order = np.argsort(-gaps)[:3]
    return [float((s[i] + s[i + 1]) / 2) for i in order if gaps[i] >= 2e-2]


@pytest.mark.parametrize("key", ["max_q_cls", "min_q_cls"])
def test_detect_records_equal_postprocess_of_the_raw_outputs(ctx, key):
    """opd_detr_detect_frames at 128 queries x 128 rows and at 4 x 3: label, query index and compaction order of every record equal the
    oracle's post_process_object_detection on the handle's own logits and boxes; score and box within the kernel test's bounds."""
    c = ctx(key)
    lib = _capi.load_library()
    q = ARCHS[key][2]
    oracle_scores = _softmax(c.oracle[0])[..., :-1].max(-1)
    thresholds = _thresholds(oracle_scores)
    assert thresholds, "no gap of 2e-2 in the oracle's scores"
    logits, boxes, _ = c.raw
    kept = 0
    for thr in thresholds:
        assert np.abs(oracle_scores - thr).min() >= 1e-2   # on the oracle, before anything is compared: no record is set aside
        want = O.post_process_object_detection(logits, boxes, thr, [(H, W)] * 2)
        recs, counts = np.zeros((2, q), DET), np.full(2, -7, np.int32)
        ptrs = (C.c_void_p * 2)(*[f.ctypes.data for f in c.frames])
        rc = lib.opd_detr_detect_frames(C.c_void_p(c.det.model), ptrs, _capi.OPD_MEM_HOST, 2, H, W, H, W, thr,
                                        C.cast(C.c_void_p(recs.ctypes.data), C.POINTER(_capi.OpdDet)), C.cast(C.c_void_p(counts.ctypes.data), C.POINTER(C.c_int32)))
        _capi.check(rc, "opd_detr_detect_frames")
        compare_records(recs, counts, want)
        assert counts.tolist() == [int((oracle_scores[b] > thr).sum()) for b in range(2)]
        kept += int(counts.sum())
    assert kept >= 2
    _redzones_intact(c.det)


def _sig(dets):
    return [(d.bbox, d.confidence, d.class_id, d.camera_coords, d.query_index, None if d.features is None else np.asarray(d.features).tobytes()) for d in dets]


def test_stride_128_fused_feature_call_and_device_nms(ctx):
    """128 queries = a record stride of 128, the most the fused calls and person_nms_kernel take.  (a) detect + features in one call equals
    detect followed by opd_detr_roi_features bit for bit, at model resolution and through the device resize; (b) suppression on the device
    returns the Detection lists suppression on the host returns, through detect, detect_batch and both fused feature calls, also at the IoU
    limit where nothing is suppressed.  Threshold 0.05, so that suppression has something to drop."""
    path = ctx("max_q_cls").path
    frame_sets = [structured_frames(3, H, W, seed=41), structured_frames(3, 160, 200, seed=41)]   # (the second: resized on the device to 256 x 320)
    dets = {}
    try:
        for name, kw in (("lists", {}), ("stacked", {"frame_lists": False}), ("device_nms", {"device_nms": True})):
            dets[name] = _poisoned(path, max_batch=2, max_size=(H, W), resize=True, confidence_threshold=0.05, **kw)
        assert dets["lists"].num_queries == 128
        n_feat, removed = 0, 0
        for frames in frame_sets:
            assert dets["lists"]._frame_list_target(frames) == (H, W)
            for frame in frames[:2] + frames[:1]:                              # (the last call replays the graph on re-used buffers)
                (da, fa), (db, fb) = dets["lists"].detect_with_features(frame), dets["stacked"].detect_with_features(frame)
                assert _sig(da) == _sig(db)
                np.testing.assert_array_equal(np.asarray(fa), np.asarray(fb))
                n_feat += len(da)
                if len(da):
                    assert np.allclose(np.linalg.norm(fa, axis=1), 1.0, atol=1e-4)
            for limit in (1.0, 0.4):                                           # (ends on the default, which the next frames' feature calls use)
                for d in dets.values():
                    d.nms_threshold = limit
                want = dets["lists"].detect(frames[0])
                assert _sig(dets["device_nms"].detect(frames[0])) == _sig(want)
                got_b, want_b = dets["device_nms"].detect_batch(frames), dets["lists"].detect_batch(frames)   # 3 frames, max_batch = 2: two chunks
                assert [_sig(g) for g in got_b] == [_sig(w) for w in want_b] and len(got_b) == 3
                for kind in ("encoder", "color"):
                    (gd, gf), (wd, wf) = dets["device_nms"].detect_with_features(frames[0], features=kind), dets["lists"].detect_with_features(frames[0], features=kind)
                    assert _sig(gd) == _sig(wd) and np.array_equal(np.asarray(gf), np.asarray(wf)), (kind, limit)
                removed += (1 if limit == 1.0 else -1) * len(want)
        assert n_feat >= 2, f"the test frames give {n_feat} person detections at threshold 0.05: nothing to compare"
        assert removed > 0, "suppression dropped nothing on these frames"
        for d in dets.values():
            _redzones_intact(d)
    finally:
        for d in dets.values():
            d.close()
