"""The int8 HIP kernels on weight blobs OTHER than the shipped one (tests/model_variants.py), against the oracle run on a .yfm that states the same
weights -- bit for bit, no tolerance: heads through every kernel set, every fused stage through the dump, the 160x160 band kernels, the fused decode
and camera entries, the refusal of a blob outside the admission bound through the ABI, and the rounding switched before and after init.
tests/test_model_variants_host.py checks, from the oracle alone, that these variants are informative."""
import numpy as np
import pytest

import model_variants as mv

pytestmark = pytest.mark.gpu

ROUNDINGS = [0, 1, 2, 3, 0x101, 0x103, mv.FP32]                # reference kernels | sign-free dense epilogue | the same roundings on the generic kernels | fp32 set
VARIANTS = mv.all_admitted()
REFUSED = mv.bias_edges(refused=True)
N_TILED = (513, 1027)                                          # ragged counts above 512: the batched shape with its paired tail


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


@pytest.fixture(scope="module")
def frames(torch_cuda):
    x = mv.variant_frames()
    tiled = {n: np.random.default_rng(n).integers(0, x.shape[0], n) for n in N_TILED}
    for n in tiled:
        tiled[n][:x.shape[0]] = np.arange(x.shape[0])
    return dict(x=x, d_x=torch_cuda.from_numpy(x).cuda(), tiled=tiled, d_tiled={n: torch_cuda.from_numpy(x[i]).cuda() for n, i in tiled.items()})


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    """variant -> (blob, oracle of the .yfm that states the same weights), each built once"""
    from oracle.oracle import Oracle
    d, cache = tmp_path_factory.mktemp("variants"), {}

    def get(v):
        if v.name not in cache:
            blob, path = v.build(d)
            cache[v.name] = (np.frombuffer(blob, np.uint8).copy(), Oracle(path))
        return cache[v.name]
    return get


_BOUND = dict(name=None, refs={})                               # the variant the session's network is bound to; the oracle's answers for it


@pytest.fixture(scope="module")
def bound(network, built):
    """bind(v, rounding): the session's network initialised from the variant's blob with the rounding in force.  A variant stays bound over its consecutive
    test ids (one ai_network_init per variant, the rounding switched on the ready network); whatever a test did, the module leaves the session's network
    on the shipped blob, the reference rounding and the automatic shape.
    INVARIANT: _BOUND names what the session's network is bound to.  bind() is the only place that sets it, and it sets it only after ai_network_init
    succeeded (a failed init leaves it None, so the next id initialises again instead of switching roundings on a network that never came up).  Every test
    of this module that calls network.init() on its own must end in _restore(network) (try/finally), which clears _BOUND and puts the shipped blob back;
    the ids of one variant are consecutive because pytest varies the topmost parametrize fastest."""
    def bind(v, rounding):
        network.configure(-1, -1)
        if _BOUND["name"] != v.name:
            _BOUND.update(name=None, refs={})
            network.set_requant_rounding(0)
            network.init(weights=built(v)[0])
            _BOUND["name"] = v.name
        network.set_requant_rounding(rounding)
        assert network.requant_rounding == rounding
        return built(v)[1]
    try:
        yield bind
    finally:
        _restore(network)
        network.configure(-1, -1)


def _restore(network):
    """the shipped blob and the reference rounding again, whatever state a test, a refused init or a refused switch left"""
    _BOUND.update(name=None, refs={})
    network.set_requant_rounding(0)
    network.init()


def _run_device(torch, network, d_in, n, canary=77):
    d_out = torch.full((n + 1, 7, 7, 18), canary, dtype=torch.int8, device="cuda")
    network.run_device(d_in.data_ptr(), d_out.data_ptr(), n)
    torch.cuda.synchronize()
    got = d_out.cpu().numpy()
    assert (got[n] == canary).all(), "wrote past the last frame"
    return got[:n]


def _assert_heads(got, ref, what):
    d = mv.first_difference(got.reshape(got.shape[0], -1), ref.reshape(ref.shape[0], -1), (7, 7, 18))
    assert d is None, f"{what}: head differs first at (frame, y, x, channel) = {d[:4]}: got {d[4]}, oracle {d[5]}"


def _reference(orc, frames, variant):
    """(heads, per-op dump) of the WHOLE frame set from the oracle -- the set on which tests/test_model_variants_host.py shows that every amplified conv
    reaches both clamps -- kept while the variant stays bound (ties_up and ties_up+generic are one oracle variant)"""
    if variant not in _BOUND["refs"]:
        _BOUND["refs"][variant] = orc.run(frames["x"], dump=True, threads=16, variant=variant)
    return _BOUND["refs"][variant]


def _assert_stages(torch, network, orc, frames, variant, what):
    sizes, offs, shapes = mv.dump_layout()
    head_ref, dump_ref = _reference(orc, frames, variant)
    n = head_ref.shape[0]
    d_out = torch.zeros((n, 7, 7, 18), dtype=torch.int8, device="cuda")
    d_dump = torch.zeros((n, network.dump_bytes()), dtype=torch.int8, device="cuda")
    network.run_device(frames["d_x"].data_ptr(), d_out.data_ptr(), n, None, d_dump.data_ptr())
    torch.cuda.synchronize()
    dump, off = d_dump.cpu().numpy(), 0
    for name, op in mv.STAGES:
        d = mv.first_difference(dump[:, off:off + sizes[op]], dump_ref[:, offs[op]:offs[op] + sizes[op]], shapes[op])
        assert d is None, f"{what}: stage {name} (tflite op {op}) differs first at (frame, y, x, channel) = {d[:4]}: got {d[4]}, oracle {d[5]}"
        off += sizes[op]
    assert off == network.dump_bytes()
    _assert_heads(d_out.cpu().numpy(), head_ref, what + " (dump build)")


@pytest.mark.parametrize("rounding", ROUNDINGS, ids=[mv.rounding_name(r) for r in ROUNDINGS])
@pytest.mark.parametrize("v", VARIANTS, ids=[v.name for v in VARIANTS])
def test_heads_and_stages_equal_the_oracle(yf, network, bound, frames, torch_cuda, v, rounding):
    """Every variant the host admits, every kernel set: the heads of the frame set through run_device (one frame per workgroup, canary frame behind the
    batch), through ai_network_run on host arrays, and of the set tiled to 513 and 1027 frames (batched shape, paired tail); and all STAGES tensors of
    every frame of the set through the dump build against the oracle's per-op dump -- for amplify(conv) the clamped stage itself is compared, not only what survives to the head.
    A (variant, rounding) pair the host does NOT admit (YF_ROUND_FP32 on some bias_edge blobs) is refused by the switch with a latched error, and
    the network goes on computing the rounding that was in force."""
    torch = torch_cuda
    what = f"{v.name}, rounding {mv.rounding_name(rounding)}"
    variant = mv.ROUNDINGS[rounding & 0xFF][1]
    x = frames["x"]
    if not v.admitted(rounding):
        orc = bound(v, 1)
        with pytest.raises(yf.NetworkError) as ei:
            network.set_requant_rounding(rounding)
        assert (ei.value.type, ei.value.code) == (0x11, 0x12) and network.requant_rounding == 1, what
        _assert_heads(_run_device(torch, network, frames["d_x"], x.shape[0]), orc.run(x, threads=16, variant=1), what + " (refused: still ties_up)")
        return
    orc = bound(v, rounding)
    assert "F=1,NW=8" in network.kernel_name_for(x.shape[0]) and "F=2,NW=8" in network.kernel_name_for(N_TILED[0])
    assert ("fp32 requantisation" in network.kernel_name) == (rounding == mv.FP32) and (rounding == mv.FP32 or ("sign-free" in network.kernel_name) == (rounding in (1, 2, 3)))
    ref = _reference(orc, frames, variant)[0]
    _assert_heads(_run_device(torch, network, frames["d_x"], x.shape[0]), ref, what)
    _assert_heads(network.run(x), ref, what + " (ai_network_run)")
    for n, idx in frames["tiled"].items():
        _assert_heads(_run_device(torch, network, frames["d_tiled"][n], n), ref[idx], what + f" (n = {n})")
    _assert_stages(torch, network, orc, frames, variant, what)


DW_VARIANTS = [mv.jitter(1)] + [mv.amplify(op) for op in mv.DW_OPS] + [mv.uniform(op, val) for op in mv.DW_OPS for val in (127, -128)]


@pytest.mark.parametrize("rounding", [0, 1], ids=["ref", "ties_up"])
@pytest.mark.parametrize("v", DW_VARIANTS, ids=[v.name for v in DW_VARIANTS])
def test_160x160_band_kernels_equal_the_oracle(network, bound, torch_cuda, v, rounding):
    """Band seams and halos are where the three band kernels differ from the fused one: jitter, amplify and uniform(+127 / -128) of every depthwise conv
    (sum(w) at its extremes against the halo fill) on the frames of test_160x160_band_edges, against the oracle at 160x160."""
    torch = torch_cuda
    x = mv.band_edge_frames_160()
    orc = bound(v, rounding)
    ref = orc.run(x, threads=16, variant=mv.ROUNDINGS[rounding][1])
    d_in = torch.from_numpy(x).cuda()
    d_out = torch.full((x.shape[0] + 1, 20, 20, 18), 77, dtype=torch.int8, device="cuda")
    network.run_device_hw(160, 160, d_in.data_ptr(), d_out.data_ptr(), x.shape[0])
    torch.cuda.synchronize()
    got = d_out.cpu().numpy()
    d = mv.first_difference(got[:-1].reshape(x.shape[0], -1), ref.reshape(x.shape[0], -1), (20, 20, 18))
    assert d is None and (got[-1] == 77).all(), f"{v.name}: 160x160 head differs first at (frame, y, x, channel) = {d and d[:4]}: got {d and d[4]}, oracle {d and d[5]}"


def _records(yf, d_d, d_c, n, cap):
    buf, counts = d_d.cpu().numpy().view(yf.DET_DTYPE).reshape(n, cap), d_c.cpu().numpy()
    return counts, [[(int(d["anchor"]), int(d["row"]), int(d["col"]), int(d["q_conf"]), float(d["conf"]), int(d["x1"]), int(d["y1"]), int(d["x2"]), int(d["y2"]))
                     for d in buf[f, :min(int(counts[f]), cap)]] for f in range(n)]


FUSED_VARIANTS = [mv.jitter(1), mv.jitter(2), mv.amplify(53)]


@pytest.mark.parametrize("v", FUSED_VARIANTS, ids=[v.name for v in FUSED_VARIANTS])
def test_fused_decode_and_camera_entries(yf, network, bound, frames, torch_cuda, v):
    """yf_network_run_decode_device (modes 0, 1, 2) and yf_network_run_camera_device on foreign weights: heads equal to the oracle's, records equal to the
    oracle's decode of those heads (decode_py / decode_c), as the shipped-blob tests of the two entries check them."""
    torch = torch_cuda
    orc = bound(v, 0)
    n = N_TILED[0]
    idx, d_x = frames["tiled"][n], frames["d_tiled"][n]
    ref = orc.run(frames["x"], threads=16)[idx]
    cap, n_det = 8, 0
    for mode in (0, 1, 2):
        ws, hs = (410 / 56.0, 362 / 56.0) if mode == 0 else (1.0, 1.0)
        d_h = torch.zeros((n, 7, 7, 18), dtype=torch.int8, device="cuda")
        d_d = torch.zeros((n, cap, 28), dtype=torch.uint8, device="cuda")
        d_c = torch.full((n,), -1, dtype=torch.int32, device="cuda")
        network.run_decode_device(d_x.data_ptr(), d_h.data_ptr(), n, d_d.data_ptr(), d_c.data_ptr(), cap, mode, ws, hs)
        torch.cuda.synchronize()
        _assert_heads(d_h.cpu().numpy(), ref, f"{v.name}, run_decode_device mode {mode}")
        counts, got = _records(yf, d_d, d_c, n, cap)
        for f in range(n):
            want = orc.decode_py(ref[f], f, ws, hs) if mode == 0 else orc.decode_c(ref[f], f, host_x86=(mode == 2))
            assert counts[f] == len(want) and got[f] == [tuple(d[1:]) for d in want][:cap], (v.name, mode, f)
            n_det += len(want)
    assert n_det > 0
    raw = np.random.default_rng(34).integers(0, 256, (131, 112 * 112 * 2), dtype=np.uint8)
    raw[0], raw[1] = 0, 255
    cam_ref = orc.run(np.stack([orc.prepare_rgb565(r) for r in raw]), threads=16)
    d_raw = torch.from_numpy(raw).cuda()
    d_h = torch.full((132, 7, 7, 18), 9, dtype=torch.int8, device="cuda")
    d_d = torch.zeros((131, cap, 28), dtype=torch.uint8, device="cuda")
    d_c = torch.zeros((131,), dtype=torch.int32, device="cuda")
    network.run_camera_device(d_raw.data_ptr(), d_h.data_ptr(), 131, d_d.data_ptr(), d_c.data_ptr(), cap, yf.YF_DECODE_FW)
    torch.cuda.synchronize()
    heads = d_h.cpu().numpy()
    _assert_heads(heads[:131], cam_ref, f"{v.name}, run_camera_device")
    assert (heads[131] == 9).all()
    counts, got = _records(yf, d_d, d_c, 131, cap)
    for f in range(131):
        want = orc.decode_c(cam_ref[f], f)
        assert counts[f] == len(want) and [g[:3] + g[5:] for g in got[f]] == [(d[1], d[2], d[3], d[6], d[7], d[8], d[9]) for d in want][:cap], (v.name, f)


@pytest.mark.parametrize("v", REFUSED, ids=[v.name for v in REFUSED])
def test_a_blob_outside_the_admission_bound_is_refused_through_the_abi(yf, network, oracle, bound, frames, tmp_path, v):
    """The 2^29 twin of each bias_edge: ai_network_init fails with the reference's error convention (AI_ERROR_INIT_FAILED / NETWORK_WEIGHTS latched, reading
    resets it), nothing is launched (ai_network_run refuses: INVALID_STATE / MISSED_INIT), and the following init on the shipped blob runs and equals the
    oracle."""
    blob = np.frombuffer(v.build(tmp_path)[0], np.uint8).copy()
    x = frames["x"][:9]
    try:
        with pytest.raises(yf.NetworkError) as ei:
            network.init(weights=blob)
        assert (ei.value.type, ei.value.code) == (0x30, 0x12) and "table preparation failed (code 3)" in ei.value.text
        assert network.get_error() == (0, 0)
        with pytest.raises(yf.NetworkError) as ei:
            network.run(x)
        assert (ei.value.type, ei.value.code) == (0x11, 0x30)
    finally:
        _restore(network)
    assert np.array_equal(network.run(x), oracle.run(x))


SWITCH_VARIANTS = [mv.jitter(2), mv.amplify(15)]


@pytest.mark.parametrize("rounding", ROUNDINGS[1:], ids=[mv.rounding_name(r) for r in ROUNDINGS[1:]])
@pytest.mark.parametrize("v", SWITCH_VARIANTS, ids=[v.name for v in SWITCH_VARIANTS])
def test_rounding_selected_before_and_after_init(network, built, frames, torch_cuda, v, rounding):
    """yf_network_set_requant_rounding on a ready network prepares the new tables from the blob BOUND AT INIT (the caller's), not from the library's:
    selected before init(weights=blob) and after it, both orders equal the oracle on the variant -- and differ from the shipped model's heads."""
    torch = torch_cuda
    blob, orc = built(v)
    x = frames["x"]
    variant = mv.ROUNDINGS[rounding & 0xFF][1]
    ref = orc.run(x, threads=16, variant=variant)
    from oracle.oracle import Oracle
    assert not np.array_equal(ref, Oracle().run(x, threads=16, variant=variant))
    try:
        network.set_requant_rounding(rounding)                # before: on the shipped blob, then init binds the caller's
        network.init(weights=blob)
        assert network.requant_rounding == rounding
        _assert_heads(_run_device(torch, network, frames["d_x"], x.shape[0]), ref, f"{v.name}: {mv.rounding_name(rounding)} selected before init")
        network.set_requant_rounding(0)
        network.init(weights=blob)                            # after: init under the reference rounding, then the switch
        _assert_heads(_run_device(torch, network, frames["d_x"], x.shape[0]), orc.run(x, threads=16), f"{v.name}: reference rounding")
        network.set_requant_rounding(rounding)
        _assert_heads(_run_device(torch, network, frames["d_x"], x.shape[0]), ref, f"{v.name}: {mv.rounding_name(rounding)} selected after init")
        _assert_heads(network.run(x), ref, f"{v.name}: {mv.rounding_name(rounding)} selected after init (ai_network_run)")
    finally:
        _restore(network)


@pytest.mark.parametrize("in_force", [0, 1, 3], ids=["ref", "ties_up", "single"])
def test_a_switch_to_a_rounding_that_refuses_the_bound_blob(yf, network, built, frames, torch_cuda, in_force):
    """A blob every integer rounding admits and YF_ROUND_FP32 refuses (one channel's acc_max * fs just reaches 2^21): the switch after init returns the
    latched error, the rounding in force stays, and the next run still equals the oracle for it.  Its twin on the admitted side of the bound switches
    to the fp32 kernel set and equals the oracle's fp32 variant; init under YF_ROUND_FP32 refuses the first and admits the twin."""
    torch = torch_cuda
    x = frames["x"]
    bad, ok = mv.fp32_edge(refused=True), mv.fp32_edge()
    assert bad.admitted(in_force) and not bad.admitted(mv.FP32) and ok.admitted(mv.FP32)
    (blob, orc), (blob_ok, orc_ok) = built(bad), built(ok)
    try:
        network.set_requant_rounding(in_force)
        network.init(weights=blob)
        with pytest.raises(yf.NetworkError) as ei:
            network.set_requant_rounding(mv.FP32)
        assert (ei.value.type, ei.value.code) == (0x11, 0x12) and network.get_error() == (0, 0) and network.requant_rounding == in_force
        _assert_heads(_run_device(torch, network, frames["d_x"], x.shape[0]), orc.run(x, threads=16, variant=mv.ROUNDINGS[in_force][1]), f"{bad.name}: after the refused switch")
        network.init(weights=blob_ok)
        network.set_requant_rounding(mv.FP32)
        assert "fp32 requantisation" in network.kernel_name
        _assert_heads(_run_device(torch, network, frames["d_x"], x.shape[0]), orc_ok.run(x, threads=16, variant=3), f"{ok.name}: fp32")
        with pytest.raises(yf.NetworkError) as ei:              # init under the fp32 rounding: the refused twin fails it, the admitted one initialises
            network.init(weights=blob)
        assert (ei.value.type, ei.value.code) == (0x30, 0x12)
        network.init(weights=blob_ok)
        _assert_heads(network.run(x), orc_ok.run(x, threads=16, variant=3), f"{ok.name}: fp32 at init")
    finally:
        _restore(network)
