"""Re-quantised variants of the shipped model as .yfm images -- TEST INFRASTRUCTURE (tests/test_model_file_host.py, tests/test_model_file_gpu.py).

Every variant is oracle/model/yoloface_int8.yfm with other numbers in it, written by the package's own writer, so the library
(yf_network_init_model) and the oracle (Oracle(path)) are given the same bytes:
  S  the shipped bytes
  A  the activations re-quantised: every activation tensor's scale times a factor in [0.8, 1.25], its zero point moved by up to +-12 (clipped to
     int8); the input tensor left alone; the converter's constraints re-imposed (a PAD or pool output equals its input, concat inputs equal the
     concat output); every bias re-derived as round(b_q * old_scale / new_scale) with the new s_in * s_w
  W  A plus every per-channel filter scale times a factor in [0.9, 1.1], biases re-derived
  O  the shipped model with only the output tensor's scale and zero point changed (the last convolution's requantisation follows from them;
     nothing else in the file depends on them): isolates the decode tables
The seeds were chosen on the CPU so that the host admits each variant under the reference, ties_up and fp32 roundings and the oracle's heads on
the golden frames differ from the shipped model's; tests/test_model_file_host.py asserts both.
"""
import importlib
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIPPED = os.path.join(ROOT, "oracle", "model", "yoloface_int8.yfm")
model_file = importlib.import_module("stm32h7-yolo_amd.model_file")

PAD, CONV, DWCONV, MAXPOOL, CONCAT = 34, 3, 4, 17, 2
SEEDS = {"A": 1, "W": 1, "O": 1}      # W = A (same seed: the same activations) plus the filter scales
NAMES = ("S", "A", "W", "O")
_CACHE = {}


def shipped_bytes():
    return open(SHIPPED, "rb").read()


def _f32(x):
    return np.asarray(x, np.float32)


def _activations(m):
    return [i for i, t in enumerate(m["tensors"]) if t["data"] is None]


def _requantise_activations(m, rng):
    T = m["tensors"]
    for i in _activations(m):
        if i == m["input"]:
            continue
        T[i]["scale"] = _f32(T[i]["scale"] * np.float32(rng.uniform(0.8, 1.25)))
        T[i]["zp"] = int(np.clip(T[i]["zp"] + rng.integers(-12, 13), -128, 127))
    for o in m["ops"]:                               # the converter's constraints, in graph order (a pool's input is final before its output is copied)
        if o["op"] in (PAD, MAXPOOL):
            T[o["out"]]["scale"], T[o["out"]]["zp"] = T[o["ins"][0]]["scale"].copy(), T[o["ins"][0]]["zp"]
    for o in m["ops"]:
        if o["op"] == CONCAT:
            for i in o["ins"][:2]:
                T[i]["scale"], T[i]["zp"] = T[o["out"]]["scale"].copy(), T[o["out"]]["zp"]


def _rederive_biases(m, old):
    """bias_q' = round(bias_q * old_scale / new_scale), new_scale = fl32(s_in * s_w[c]) of the model as it stands"""
    T = m["tensors"]
    for o in m["ops"]:
        if o["op"] not in (CONV, DWCONV):
            continue
        tin, tw, tb = o["ins"]
        new = _f32(_f32(T[tin]["scale"][0]) * _f32(T[tw]["scale"]))
        old_scale = old["tensors"][tb]["scale"].astype(np.float64)
        T[tb]["data"] = np.rint(old["tensors"][tb]["data"].astype(np.float64) * old_scale / new.astype(np.float64)).astype(np.int32)
        T[tb]["scale"] = new


def build(name, seed=None):
    """The bytes of variant `name` (S, A, W, O)."""
    if name == "S":
        return shipped_bytes()
    key = (name, seed)
    if key in _CACHE:
        return _CACHE[key]
    old = model_file.load_yfm(SHIPPED)
    m = model_file.load_yfm(SHIPPED)
    rng = np.random.default_rng(SEEDS[name] if seed is None else seed)
    if name in ("A", "W"):
        _requantise_activations(m, rng)
        if name == "W":
            for o in m["ops"]:
                if o["op"] in (CONV, DWCONV):
                    w = m["tensors"][o["ins"][1]]
                    w["scale"] = _f32(w["scale"] * rng.uniform(0.9, 1.1, w["scale"].shape).astype(np.float32))
        _rederive_biases(m, old)
    elif name == "O":
        t = m["tensors"][m["output"]]
        t["scale"] = _f32(t["scale"] * np.float32(rng.uniform(0.8, 1.25)))
        t["zp"] = int(np.clip(t["zp"] + rng.integers(-12, 13), -128, 127))
    else:
        raise ValueError(name)
    _CACHE[key] = model_file.write_yfm(m)
    return _CACHE[key]


def write(name, directory):
    """Variant `name` as a file in `directory`; its path (for Oracle(path) and Interpreter(model_path=path))."""
    path = os.path.join(str(directory), f"yoloface_int8_{name}.yfm")
    with open(path, "wb") as f:
        f.write(build(name))
    return path


def output_quantization(name):
    m = model_file.load_yfm(build(name))
    t = m["tensors"][m["output"]]
    return np.float32(t["scale"][0]), int(t["zp"])
