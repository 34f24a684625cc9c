"""Re-quantised models on the GPU: yf_network_init_model against Oracle(<the same .yfm bytes>), bit for bit -- heads through every launch form, every
fused stage through the dump build, the 160x160 band kernels, the camera entry; the decode tables of another output quantisation through the
fused decode, libyf_images and the Interpreter.  The variants are tests/requant_models.py's (tests/test_model_file_host.py shows that none of them
computes the shipped heads)."""
import importlib
import os

import numpy as np
import pytest

from conftest import ROOT, GOLDEN
import model_variants as mv
import requant_models as rm
from images_support import expect_frame

pytestmark = pytest.mark.gpu
REF, TIES_UP, FP32 = 0, 1, 0x10
ORACLE_VARIANT = {REF: 0, TIES_UP: 1, FP32: 3}
CASES = [("A", REF), ("W", REF), ("W", TIES_UP), ("W", FP32)]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


@pytest.fixture(scope="module")
def oracles(tmp_path_factory):
    from oracle.oracle import Oracle
    d = tmp_path_factory.mktemp("requant_gpu")
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = Oracle(rm.write(name, d))
        return cache[name]
    return get


@pytest.fixture(scope="module")
def frames(torch_cuda):
    """67 frames: the golden six, the real ones and noise; n = 1, 5 and 67 are prefixes of it"""
    real = np.fromfile(os.path.join(GOLDEN, "real_frames_56.bin"), np.int8).reshape(-1, 56, 56, 3)
    gold = np.fromfile(os.path.join(GOLDEN, "golden_inputs.bin"), np.int8).reshape(-1, 56, 56, 3)
    x = np.concatenate([gold, real, np.random.default_rng(67).integers(-128, 128, (67 - 6 - real.shape[0], 56, 56, 3), dtype=np.int8)])
    assert x.shape[0] == 67
    return dict(x=x, d_x=torch_cuda.from_numpy(x).cuda(), real=real)


@pytest.fixture(scope="module")
def bind(network):
    """bind(name, rounding): the session's network initialised from the variant's bytes (image: another model's, under a name of its own) with the
    rounding in force; the module leaves the network as it found it (the shipped model under the reference rounding)."""
    state = {"name": None}

    def go(name, rounding=REF, image=None):
        if state["name"] != name:
            network.set_requant_rounding(REF)
            network.init_model(rm.build(name) if image is None else image)
            state["name"] = name
        network.set_requant_rounding(rounding)
        assert network.requant_rounding == rounding
        return network
    try:
        yield go
    finally:
        network.set_requant_rounding(REF)
        network.init()


def _run(torch, network, d_in, n):
    d_out = torch.full((n + 1, 7, 7, 18), 77, dtype=torch.int8, device="cuda")
    network.run_device(d_in.data_ptr(), d_out.data_ptr(), n)
    torch.cuda.synchronize()
    got = d_out.cpu().numpy()
    assert (got[n] == 77).all(), "wrote past the last frame"
    return got[:n]


def _assert_heads(got, ref, what, shape=(7, 7, 18)):
    d = mv.first_difference(got.reshape(got.shape[0], -1), ref.reshape(ref.shape[0], -1), shape)
    assert d is None, f"{what}: head differs first at (frame, y, x, channel) = {d[:4]}: got {d[4]}, oracle {d[5]}"


def test_shipped_bytes_through_init_model_give_the_golden_heads(network, bind, frames, torch_cuda):
    bind("S")
    gold = np.fromfile(os.path.join(GOLDEN, "golden_heads.bin"), np.int8).reshape(-1, 7, 7, 18)
    _assert_heads(_run(torch_cuda, network, frames["d_x"], 6), gold, "S through yf_network_init_model")
    _assert_heads(network.run(frames["x"][:6]), gold, "S through yf_network_init_model (ai_network_run)")
    shipped = np.fromfile(os.path.join(GOLDEN, "decode_tables_f32.bin"), "<u4").reshape(2, 256)
    sig, ex, _ = network.decode_tables()
    assert np.array_equal(sig.view(np.uint32), shipped[0]) and np.array_equal(ex.view(np.uint32), shipped[1])     # the shipped tables stay the contract


@pytest.mark.parametrize("name,rounding", CASES, ids=[f"{n}-{mv.rounding_name(r)}" for n, r in CASES])
def test_requantised_model_equals_its_oracle(yf, network, bind, oracles, frames, torch_cuda, name, rounding):
    """run_device at n = 1 (the one-frame kernel), 5 (odd: an unpaired last frame) and 67 (several workgroups); the dump build at n = 2 stage by
    stage; 160x160 at n = 2; the camera entry at n = 3 -- all against Oracle(variant.yfm) in the matching oracle variant."""
    what = f"{name}, rounding {mv.rounding_name(rounding)}"
    bind(name, rounding)
    assert_network_equals_oracle(torch_cuda, network, oracles(name), ORACLE_VARIANT[rounding], frames, what, oracles("S"), fp32=rounding == FP32)


def assert_network_equals_oracle(torch, network, orc, ov, frames, what, shipped, fp32, stages_first=False):
    """The bound network against `orc` in oracle variant `ov`, bit for bit, through every launch form (the docstring above); its heads must not be
    the shipped model's.  stages_first: the dump build before the heads, so that a failure names the first wrong stage, pixel and channel rather
    than what is left of it in a head.  Also used by tests/test_quant_designs_gpu.py."""
    assert ("fp32 requantisation" in network.kernel_name) == fp32
    ref, dump_ref = orc.run(frames["x"], dump=True, threads=16, variant=ov)
    assert not np.array_equal(ref, shipped.run(frames["x"], threads=16, variant=ov))
    if stages_first:
        _assert_stages(torch, network, frames, ref, dump_ref, what)
    for n in (1, 5, 67):
        _assert_heads(_run(torch, network, frames["d_x"], n), ref[:n], f"{what}, n = {n}")
    _assert_heads(network.run(frames["x"][:5]), ref[:5], what + " (ai_network_run)")
    if not stages_first:
        _assert_stages(torch, network, frames, ref, dump_ref, what)
    _assert_160_and_camera(torch, network, orc, ov, what)


def _assert_stages(torch, network, frames, ref, dump_ref, what):
    sizes, offs, shapes = mv.dump_layout()
    d_out = torch.zeros((2, 7, 7, 18), dtype=torch.int8, device="cuda")
    d_dump = torch.zeros((2, network.dump_bytes()), dtype=torch.int8, device="cuda")
    network.run_device(frames["d_x"].data_ptr(), d_out.data_ptr(), 2, None, d_dump.data_ptr())
    torch.cuda.synchronize()
    dump, off = d_dump.cpu().numpy(), 0
    for stage, op in mv.STAGES:
        d = mv.first_difference(dump[:, off:off + sizes[op]], dump_ref[:2, offs[op]:offs[op] + sizes[op]], shapes[op])
        assert d is None, f"{what}: stage {stage} (tflite op {op}) differs first at (frame, y, x, channel) = {d[:4]}: got {d[4]}, oracle {d[5]}"
        off += sizes[op]
    assert off == network.dump_bytes()
    _assert_heads(d_out.cpu().numpy(), ref[:2], what + " (dump build)")


def _assert_160_and_camera(torch, network, orc, ov, what):
    x160 = mv.band_edge_frames_160()[:2]
    ref160 = orc.run(x160, threads=16, variant=ov)
    d_in = torch.from_numpy(x160).cuda()
    d_o = torch.full((3, 20, 20, 18), 77, dtype=torch.int8, device="cuda")
    network.run_device_hw(160, 160, d_in.data_ptr(), d_o.data_ptr(), 2)
    torch.cuda.synchronize()
    got = d_o.cpu().numpy()
    _assert_heads(got[:2], ref160, what + ", 160x160", (20, 20, 18))
    assert (got[2] == 77).all()

    raw = np.random.default_rng(3).integers(0, 256, (3, 112 * 112 * 2), dtype=np.uint8)
    cam_ref = orc.run(np.stack([orc.prepare_rgb565(r) for r in raw]), threads=16, variant=ov)
    d_raw = torch.from_numpy(raw).cuda()
    d_h = torch.full((4, 7, 7, 18), 9, dtype=torch.int8, device="cuda")
    network.run_camera_device(d_raw.data_ptr(), d_h.data_ptr(), 3)
    torch.cuda.synchronize()
    heads = d_h.cpu().numpy()
    _assert_heads(heads[:3], cam_ref, what + ", run_camera_device")
    assert (heads[3] == 9).all()


# ---------------------------------------------------------------------------------------------------------------- O: the decode tables
def _tables_of(scale, zp):
    """the test's own statement: numpy float32, the exponential as float64 exp rounded once (tests/test_model_file_host.py shows that no entry
    of O lies near a tie of that rounding)"""
    x = ((np.arange(-128, 128) - zp).astype(np.float32) * np.float32(scale)).astype(np.float32)
    e_neg, e_pos = np.exp(-x.astype(np.float64)).astype(np.float32), np.exp(x.astype(np.float64)).astype(np.float32)
    return (np.float32(1) / (np.float32(1) + e_neg)).astype(np.float32), e_pos


def _records(yf, d_d, d_c, n, cap):
    buf, counts = d_d.cpu().numpy().view(yf.DET_DTYPE).reshape(n, cap), d_c.cpu().numpy()
    return counts, [[(int(d["anchor"]), int(d["row"]), int(d["col"]), int(d["q_conf"]), float(d["conf"]), int(d["x1"]), int(d["y1"]), int(d["x2"]), int(d["y2"]))
                     for d in buf[f, :min(int(counts[f]), cap)]] for f in range(n)]


@pytest.fixture(scope="module")
def o_case(oracles, frames):
    """O's oracle with O's tables in its decode, and five real frames whose heads fire under them"""
    scale, zp = rm.output_quantization("O")
    orc = oracles("O")
    orc.sig, orc.ex = _tables_of(scale, zp)
    heads = orc.run(frames["real"], threads=16)
    firing = [i for i in range(heads.shape[0]) if orc.decode_py(heads[i])][:5]
    assert len(firing) == 5
    return dict(orc=orc, scale=scale, zp=zp, x=np.ascontiguousarray(frames["real"][firing]), heads=heads[firing])


def test_decode_tables_follow_the_models_output_quantisation(yf, network, bind, o_case, torch_cuda):
    """yf_network_run_decode_device in YF_DECODE_PY and YF_DECODE_FW at n = 5 on real frames that fire: the records of the restated decodes
    (tflite_prediction.py:43-63, yoloface.c:105-152) with O's output parameters and table values; the getter returns those tables."""
    torch = torch_cuda
    bind("O")
    orc, x, ref = o_case["orc"], o_case["x"], o_case["heads"]
    sig, ex, ident = network.decode_tables()
    assert np.array_equal(sig.view(np.uint32), orc.sig.view(np.uint32)) and np.array_equal(ex.view(np.uint32), orc.ex.view(np.uint32))
    interp = importlib.import_module("stm32h7-yolo_amd.interpreter")
    d_x, cap, n_det = torch.from_numpy(x).cuda(), 16, 0
    for mode in (yf.YF_DECODE_PY, yf.YF_DECODE_FW):
        ws, hs = (410 / 56.0, 362 / 56.0) if mode == yf.YF_DECODE_PY else (1.0, 1.0)
        d_h = torch.zeros((5, 7, 7, 18), dtype=torch.int8, device="cuda")
        d_d = torch.zeros((5, cap, 28), dtype=torch.uint8, device="cuda")
        d_c = torch.full((5,), -1, dtype=torch.int32, device="cuda")
        network.run_decode_device(d_x.data_ptr(), d_h.data_ptr(), 5, d_d.data_ptr(), d_c.data_ptr(), cap, mode, ws, hs)
        torch.cuda.synchronize()
        _assert_heads(d_h.cpu().numpy(), ref, f"O, run_decode_device mode {mode}")
        counts, got = _records(yf, d_d, d_c, 5, cap)
        for f in range(5):
            want = orc.decode_py(ref[f], f, ws, hs) if mode == yf.YF_DECODE_PY else orc.decode_c(ref[f], f)
            assert counts[f] == len(want) and got[f] == [tuple(d[1:]) for d in want][:cap], (mode, f)
            n_det += len(want)
            if mode == yf.YF_DECODE_PY:           # and the numpy mirror of the script, given the output parameters
                boxes = interp.decode_boxes(ref[f], w_scale=ws, h_scale=hs, output_scale=o_case["scale"], output_zero_point=o_case["zp"])
                assert boxes.tolist() == [list(d[6:]) for d in want], f
    assert n_det >= 10
    # the stand-alone decode of existing heads reads the same tables
    d_h = torch.from_numpy(ref).cuda()
    d_d = torch.zeros((5, cap, 28), dtype=torch.uint8, device="cuda")
    d_c = torch.full((5,), -1, dtype=torch.int32, device="cuda")
    network.decode_device(d_h.data_ptr(), 5, d_d.data_ptr(), d_c.data_ptr(), cap, yf.YF_DECODE_PY)
    torch.cuda.synchronize()
    counts, got = _records(yf, d_d, d_c, 5, cap)
    assert all(got[f] == [tuple(d[1:]) for d in orc.decode_py(ref[f], f)][:cap] for f in range(5))


def _detect_reference(ptq, orc, imgs, size):
    out = []
    for i, img in enumerate(imgs):
        frame = expect_frame(ptq, img, 0, size)
        head = orc.run(frame[None], threads=4)[0]
        h, w = img.shape[:2]
        recs = orc.decode_py(head, i, np.float32(w / float(size)), np.float32(h / float(size)), max_dets=3 * (size // 8) ** 2)
        out.append([list(d[6:]) for d in recs])
    return out


def test_images_detect_on_a_model_file_and_back(yf, network, bind, oracles, o_case, torch_cuda):
    """images.detect on a small ragged batch at 56 and at 160 on a network initialised from O: the records of O's oracle under O's tables.  Then
    the process's network goes back to the shipped model and libyf_images decodes with the shipped tables again (the id check), and a decode
    that takes no network follows yf_images_set_decode_tables."""
    torch = torch_cuda
    images = importlib.import_module("stm32h7-yolo_amd.images")
    ptq = importlib.import_module("stm32h7-yolo_amd.ptq")
    rgb = (o_case["x"].astype(np.int16) + 128).astype(np.uint8)
    imgs = [np.ascontiguousarray(ptq.resize_linear_u8(rgb[i], w, h)[..., ::-1]) for i, (w, h) in enumerate([(56, 56), (97, 61), (160, 200)])]
    shipped = oracles("S")
    seen = {}
    for name, orc in (("O", o_case["orc"]), ("S", shipped), ("O", o_case["orc"])):           # O, back to the shipped model, and O again
        if name == "S":
            network.set_requant_rounding(REF)
            network.init()                                                                    # (bind's cache is told below)
        else:
            network.init_model(rm.build("O"))
        ids = network.decode_tables()[2]
        for size in (56, 160):
            got = [b.tolist() for b in images.detect(network, imgs, size=size)]
            want = _detect_reference(ptq, orc, imgs, size)
            assert got == want, (name, size)
            seen[(name, size)] = sum(len(b) for b in want)
        seen[name] = ids
    assert seen["O"] != seen["S"] and seen[("O", 56)] > 0 and seen[("S", 56)] > 0
    # no network in the call: the pair last set decides.  detect has just set O's; decode O's heads, then set the shipped pair and decode again
    heads = o_case["heads"]
    d_h = torch.from_numpy(heads).cuda()
    desc = np.zeros(5, images.IMAGE_DTYPE)
    desc["height"], desc["width"], desc["row_stride"] = 56, 56, 168
    d_desc = torch.from_numpy(desc.view(np.uint8)).cuda()
    cap = 147

    def decode_no_network():
        d_d = torch.zeros((5, cap, 28), dtype=torch.uint8, device="cuda")
        d_c = torch.full((5,), -1, dtype=torch.int32, device="cuda")
        images.decode_ragged_device(d_h.data_ptr(), d_desc.data_ptr(), 5, d_d.data_ptr(), d_c.data_ptr(), cap)
        torch.cuda.synchronize()
        return _records(yf, d_d, d_c, 5, cap)[1]
    assert all(decode_no_network()[f] == [tuple(d[1:]) for d in o_case["orc"].decode_py(heads[f], f)] for f in range(5))
    network.set_requant_rounding(REF)
    network.init()
    images.set_decode_tables(*network.decode_tables())
    assert all(decode_no_network()[f] == [tuple(d[1:]) for d in shipped.decode_py(heads[f], f)] for f in range(5))
    network.init_model(rm.build("S"))                # leave what bind believes is bound consistent: S computes the shipped model
    bind("S")


def test_interpreter_loads_a_model_file(yf, network, bind, oracles, frames, tmp_path):
    """Interpreter(model_path=<variant .yfm>): the oracle's head for one frame, the variant's output quantisation in get_output_details; a path
    that does not exist keeps meaning the shipped model."""
    interp = importlib.import_module("stm32h7-yolo_amd.interpreter")
    path = rm.write("W", tmp_path)
    x = frames["x"][6:7]
    try:
        it = interp.Interpreter(model_path=path)
        it.allocate_tensors()
        it.set_tensor(it.get_input_details()[0]["index"], x)
        it.invoke()
        head = it.get_tensor(it.get_output_details()[0]["index"])
        _assert_heads(head, oracles("W").run(x), "Interpreter on W")
        scale, zp = rm.output_quantization("W")
        assert it.get_output_details()[0]["quantization"] == (float(scale), zp)
        assert it.get_input_details()[0]["quantization"][1] == -128
        it = interp.Interpreter(model_content=rm.build("A"))
        it.allocate_tensors()
        it.set_tensor(0, x)
        it.invoke()
        _assert_heads(it.get_tensor(100), oracles("A").run(x), "Interpreter on A (model_content)")
        it = interp.Interpreter(model_path="yoloface_int8.tflite")                         # the reference's call site: no such file here
        it.allocate_tensors()
        it.set_tensor(0, x)
        it.invoke()
        _assert_heads(it.get_tensor(100), oracles("S").run(x), "Interpreter on a path that does not exist")
        assert it.get_output_details()[0]["quantization"] == (interp.OUTPUT_SCALE, interp.OUTPUT_ZERO_POINT)
    finally:
        network.reclaim()                            # an Interpreter supersedes the session's Network object: take the instance back
        network.set_requant_rounding(REF)
        network.init_model(rm.build("S"))
        bind("S")


def test_refused_model_leaves_the_network_as_it_was(yf, network, bind, oracles, frames, torch_cuda):
    """A refused image names its first mismatch through the ABI and the network goes on computing the model in force; a second init_model on an
    initialised network replaces the first."""
    bind("A")
    ref = oracles("A").run(frames["x"][:5], threads=4)
    bad = bytearray(rm.build("W"))
    bad[24 + 44 * 104 + 52 * 10 + 24] = 1                                                     # op 10: stride_w 2 -> 1
    with pytest.raises(yf.NetworkError) as ei:
        network.init_model(bytes(bad))
    assert ei.value.type == 0x30 and "op 10: stride_w is 1, expected 2" in ei.value.text
    with pytest.raises(yf.NetworkError) as ei:
        network.init_model(rm.build("W")[:1000])
    assert ei.value.type == 0x30 and "bytes" in ei.value.text
    m = rm.model_file.load_yfm(rm.shipped_bytes())               # admitted by the parser, refused by the table builder: before anything is torn down
    m["tensors"][51]["scale"] = (m["tensors"][51]["scale"] * np.float32(2.0 ** -24)).astype(np.float32)
    with pytest.raises(yf.NetworkError) as ei:
        network.init_model(rm.model_file.write_yfm(m))
    assert (ei.value.type, ei.value.code) == (0x30, 0x12) and "outside what the kernels compute exactly" in ei.value.text
    _assert_heads(_run(torch_cuda, network, frames["d_x"], 5), ref, "A after three refused images")
    network.init_model(rm.build("W"))
    _assert_heads(_run(torch_cuda, network, frames["d_x"], 5), oracles("W").run(frames["x"][:5], threads=4), "W after A")
    network.init_model(rm.build("S"))
    bind("S")
