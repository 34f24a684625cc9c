"""Model files of the int8 network: the .yfm pack (what yf_network_init_model and the oracle read), the conversion from a .tflite, and the
.yfw pack of a float model (what yf_network_fp16_init and the calibration library read; layout at read_yfw).

.yfm layout (little endian):
  header  : 'YFM1', u32 n_tensors, u32 n_ops, u32 input_tensor, u32 output_tensor, u32 data_bytes
  tensor  : i32 shape[4], u32 type(0=i8,1=i32), i32 zero_point, u32 n_scales, u32 scales_off,
            i32 quantized_dimension, u32 data_off(0xFFFFFFFF=none), u32 data_bytes           (44 B)
  op      : u32 opcode, i32 inputs[3], i32 output, i32 padding, i32 stride_w, i32 stride_h,
            i32 filter_w, i32 filter_h, i32 depth_multiplier, i32 axis, u32 alpha_bits           (52 B)
  data    : scales (f32) and constant tensor bytes, each 4-byte aligned

load_yfm / write_yfm are inverses on the dict form below (write_yfm(load_yfm(b)) == b for every file write_yfm wrote); tflite_to_yfm is what
tools/gen_model.py runs to produce oracle/model/yoloface_int8.yfm.  The .tflite reader is a minimal flatbuffer reader (numpy + struct only) for the
handful of schema tables this model uses; field slot numbers follow the public TFLite schema (tensorflow/lite/schema/schema.fbs, TF 2.10; SURVEY.md
Appendix C lists the ones relied on).  Nothing here needs the native library or a GPU.
"""
import os
import re
import struct

import numpy as np

OPCODE = {"ADD": 0, "CONCATENATION": 2, "CONV_2D": 3, "DEPTHWISE_CONV_2D": 4, "MAX_POOL_2D": 17,
          "PAD": 34, "LEAKY_RELU": 98, "QUANTIZE": 114}
NO_DATA = 0xFFFFFFFF


def f32bits(x):
    return struct.unpack("<I", struct.pack("<f", float(x)))[0]


def load_yfm(path_or_bytes):
    """A .yfm file (path) or its bytes -> dict(tensors, ops, input, output).  Tensor: shape[4], type (0 int8, 1 int32), zp, qdim, scale
    (float32 array, may be empty), data (flat int8 / int32 array or None).  Op: op (opcode), ins[3] (-1 = none), out, padding, sw, sh, fw, fh,
    dm, axis, alpha_bits.  Raises ValueError on a malformed image (the library's parser, csrc/yf_model_file.c, is the one that faces untrusted bytes)."""
    b = bytes(path_or_bytes) if isinstance(path_or_bytes, (bytes, bytearray, memoryview)) else open(path_or_bytes, "rb").read()
    if len(b) < 24 or b[:4] != b"YFM1":
        raise ValueError("not a .yfm image (magic)")
    nt, no, tin, tout, nd = struct.unpack_from("<5I", b, 4)
    if 24 + 44 * nt + 52 * no + nd != len(b):
        raise ValueError("the size of the .yfm image is not what its header's counts give")
    off = 24
    data = b[24 + 44 * nt + 52 * no: 24 + 44 * nt + 52 * no + nd]
    tensors, ops = [], []
    for _ in range(nt):
        s0, s1, s2, s3, ty, zp, ns, soff, qdim, doff, dbytes = struct.unpack_from("<4iIiIIiII", b, off)
        off += 44
        if ns and soff + 4 * ns > nd or doff != NO_DATA and doff + dbytes > nd or ty > 1:
            raise ValueError("tensor record points outside the data section")
        scale = np.frombuffer(data, "<f4", ns, soff).copy() if ns else np.zeros(0, np.float32)
        val = None
        if doff != NO_DATA:
            dt = np.dtype(np.int8) if ty == 0 else np.dtype("<i4")
            val = np.frombuffer(data, dt, dbytes // dt.itemsize, doff).copy()
        tensors.append(dict(shape=[s0, s1, s2, s3], type=ty, zp=zp, qdim=qdim, scale=scale, data=val))
    for _ in range(no):
        v = struct.unpack_from("<I3ii7iI", b, off)
        off += 52
        ops.append(dict(op=v[0], ins=list(v[1:4]), out=v[4], padding=v[5], sw=v[6], sh=v[7], fw=v[8], fh=v[9], dm=v[10], axis=v[11],
                        alpha_bits=v[12]))
    return dict(tensors=tensors, ops=ops, input=tin, output=tout)


def write_yfm(model, path=None):
    """The dict form of load_yfm -> .yfm bytes (also written to `path` if given)."""
    data = bytearray()

    def put(raw):
        while len(data) % 4:
            data.append(0)
        at = len(data)
        data.extend(raw)
        return at

    trecs = []
    for t in model["tensors"]:
        scale = np.asarray(t["scale"], "<f4")
        soff = put(scale.tobytes()) if scale.size else 0
        if t["data"] is not None:
            raw = np.asarray(t["data"], np.int8 if t["type"] == 0 else "<i4").tobytes()
            doff, dbytes = put(raw), len(raw)
        else:
            doff, dbytes = NO_DATA, 0
        trecs.append(struct.pack("<4iIiIIiII", *t["shape"], t["type"], int(t["zp"]), scale.size, soff, t["qdim"], doff, dbytes))
    orecs = [struct.pack("<I3ii7iI", o["op"], *o["ins"], o["out"], o["padding"], o["sw"], o["sh"], o["fw"], o["fh"], o["dm"], o["axis"],
                         o["alpha_bits"]) for o in model["ops"]]
    while len(data) % 4:
        data.append(0)
    out = (b"YFM1" + struct.pack("<5I", len(trecs), len(orecs), model["input"], model["output"], len(data))
           + b"".join(trecs) + b"".join(orecs) + bytes(data))
    if path is not None:
        with open(path, "wb") as f:
            f.write(out)
    return out


def load_graph():
    """The graph the library is built for (csrc/gen/yf_graph_gen.h) in the dict form of load_yfm, without numbers: every op with its wiring and
    options; every tensor with shape, type, qdim, `n_scales` and `is_const`, zero point 0, no scale, and no data except the PAD ops' paddings."""
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "gen", "yf_graph_gen.h")).read()
    ops_src, tensors_src = src.split("yf_graph_ops[YF_GRAPH_N_OPS] = {")[1].split("};")[0], src.split("yf_graph_tensors[")[1].split("};")[0]
    ops = []
    for r in re.findall(r"^\s*\{(\d+), \{(-?\d+), (-?\d+), (-?\d+)\}, ((?:-?\d+, ){8})0x([0-9a-f]{8})u\},", ops_src, re.M):
        v = [int(x) for x in r[4].rstrip(", ").split(", ")]
        ops.append(dict(op=int(r[0]), ins=[int(r[1]), int(r[2]), int(r[3])], out=v[0], padding=v[1], sw=v[2], sh=v[3], fw=v[4], fh=v[5], dm=v[6],
                        axis=v[7], alpha_bits=int(r[5], 16)))
    tensors = []
    for r in re.findall(r"^\s*\{\{(\d+), (\d+), (\d+), (\d+)\}, (\d+), (\d+), (-?\d+), (\d+)\},", tensors_src, re.M):
        v = [int(x) for x in r]
        tensors.append(dict(shape=v[:4], type=v[4], zp=0, qdim=v[6], scale=np.zeros(0, np.float32), data=None, n_scales=v[7], is_const=bool(v[5])))
    pad_t = int(re.search(r"#define YF_GRAPH_PAD_TENSOR (\d+)", src).group(1))
    tensors[pad_t]["data"] = np.array([int(x) for x in re.search(r"yf_graph_paddings\[\d+\] = \{([^}]*)\}", src).group(1).split(",")], "<i4")
    n_ops, t_in, t_out = (int(re.search(r"#define YF_GRAPH_%s (\d+)" % k, src).group(1)) for k in ("N_OPS", "INPUT", "OUTPUT"))
    assert len(ops) == n_ops and len(tensors) > t_out
    return dict(tensors=tensors, ops=ops, input=t_in, output=t_out)


def graph_convs(graph=None):
    """The graph's convolutions in order: dict(op, depthwise, cin, cout, k, stride, shape) -- shape the filter's in tflite layout (OHWI / 1HWC)."""
    g = load_graph() if graph is None else graph
    out = []
    for i, o in enumerate(g["ops"]):
        if o["op"] in (OPCODE["CONV_2D"], OPCODE["DEPTHWISE_CONV_2D"]):
            sh = g["tensors"][o["ins"][1]]["shape"]
            dw = o["op"] == OPCODE["DEPTHWISE_CONV_2D"]
            out.append(dict(op=i, depthwise=dw, cin=sh[3], cout=sh[3] if dw else sh[0], k=sh[1], stride=o["sw"], shape=tuple(sh)))
    return out


def write_yfw(convs, path=None):
    """[(weights, bias, depthwise)] in tflite layout and graph order (dense OHWI, depthwise 1HWC) -> .yfw bytes:
    'YFW1', u32 n_conv, then per convolution u32 depthwise, cin, cout, k, stride, n_weights; f32 weights; f32 bias[cout].
    The channels, kernels and strides are the graph's: anything else raises ValueError."""
    g = graph_convs()
    if len(convs) != len(g):
        raise ValueError(f"{len(convs)} convs, the graph has {len(g)}")
    out = [b"YFW1", struct.pack("<I", len(g))]
    for c, ((w, b, dw), d) in enumerate(zip(convs, g)):
        w, b = np.asarray(w, "<f4"), np.asarray(b, "<f4")
        if bool(dw) != d["depthwise"] or w.size != int(np.prod(d["shape"])) or (w.ndim == 4 and tuple(w.shape) != d["shape"]) or b.size != d["cout"]:
            raise ValueError(f"conv {c}: depthwise {bool(dw)}, weights {w.shape}, bias {b.shape}; the graph has depthwise {d['depthwise']}, "
                             f"{d['shape']}, ({d['cout']},)")
        out += [struct.pack("<6I", int(d["depthwise"]), d["cin"], d["cout"], d["k"], d["stride"], w.size), w.tobytes(), b.tobytes()]
    out = b"".join(out)
    if path is not None:
        with open(path, "wb") as f:
            f.write(out)
    return out


def read_yfw(path_or_bytes):
    """A .yfw file (path) or its bytes -> [(weights, bias, depthwise)] in tflite layout, what write_yfw takes.  Raises ValueError on a file that
    is not this network (the calibration library's parser, csrc/yf_yfw.c, is the one that faces untrusted bytes)."""
    b = bytes(path_or_bytes) if isinstance(path_or_bytes, (bytes, bytearray, memoryview)) else open(path_or_bytes, "rb").read()
    g = graph_convs()
    if len(b) < 8 or b[:4] != b"YFW1" or struct.unpack_from("<I", b, 4)[0] != len(g):
        raise ValueError(f"not a .yfw image of {len(g)} convs (magic, count)")
    off, convs = 8, []
    for c, d in enumerate(g):
        want = (int(d["depthwise"]), d["cin"], d["cout"], d["k"], d["stride"], int(np.prod(d["shape"])))
        if off + 24 > len(b) or struct.unpack_from("<6I", b, off) != want:
            raise ValueError(f"conv {c}: record {struct.unpack_from('<6I', b, off) if off + 24 <= len(b) else 'truncated'}, the graph has {want}")
        off += 24
        if off + 4 * (want[5] + d["cout"]) > len(b):
            raise ValueError(f"conv {c}: weights and biases end past the file")
        w = np.frombuffer(b, "<f4", want[5], off).reshape(d["shape"]).copy()
        bias = np.frombuffer(b, "<f4", d["cout"], off + 4 * want[5]).copy()
        off += 4 * (want[5] + d["cout"])
        convs.append((w, bias, d["depthwise"]))
    if off != len(b):
        raise ValueError(f"{len(b)} bytes, the convs' counts give {off}")
    return convs


def tflite_model_to_dict(m):
    """read_tflite's result -> the dict form of load_yfm."""
    tensors = []
    for t in m["tensors"]:
        shape = (list(t["shape"]) + [1, 1, 1, 1])[:4] if len(t["shape"]) < 4 else list(t["shape"])
        tensors.append(dict(shape=shape, type={"INT8": 0, "INT32": 1}[t["type"]], zp=int(t["zero_point"][0]) if len(t["zero_point"]) else 0,
                            qdim=t["quantized_dimension"], scale=t["scale"].astype("<f4"),
                            data=None if t["data"] is None else t["data"].reshape(-1)))
    ops = []
    for op in m["ops"]:
        o = op["options"]
        ops.append(dict(op=OPCODE[op["op"]], ins=(op["inputs"] + [-1, -1, -1])[:3], out=op["outputs"][0], padding=o.get("padding", 0),
                        sw=o.get("stride_w", 1), sh=o.get("stride_h", 1), fw=o.get("filter_w", 0), fh=o.get("filter_h", 0),
                        dm=o.get("depth_multiplier", 0), axis=o.get("axis", 0), alpha_bits=f32bits(o.get("alpha", 0.0))))
    return dict(tensors=tensors, ops=ops, input=m["inputs"][0], output=m["outputs"][0])


def tflite_to_yfm(tflite_bytes):
    """The bytes of a quantised .tflite of this network -> the bytes of its .yfm pack."""
    return write_yfm(tflite_model_to_dict(read_tflite(tflite_bytes)))


def graph_header(model):
    """csrc/gen/yf_graph_gen.h: the graph yf_model_file.c requires of a model file -- every op's code, wiring and options, every tensor's shape, type,
    number of scales and quantised dimension -- as C tables (tools/gen_model.py writes it from the shipped model)."""
    T, ops = model["tensors"], model["ops"]
    out = ["/* GENERATED by tools/gen_model.py from yoloface_int8.tflite -- do not edit.",
           " * The graph of the network (SURVEY.md Appendix A) as yf_model_file.c checks a model file against it: the ops in order with their wiring and",
           " * options, and per tensor its shape, type, number of scales, quantised dimension and whether it is a constant. */",
           "#ifndef YF_GRAPH_GEN_H", "#define YF_GRAPH_GEN_H", "#include <stdint.h>", "",
           f"#define YF_GRAPH_N_OPS {len(ops)}", f"#define YF_GRAPH_INPUT {model['input']}", f"#define YF_GRAPH_OUTPUT {model['output']}", "",
           "typedef struct { uint32_t opcode; int32_t ins[3], out, padding, stride_w, stride_h, filter_w, filter_h, depth_multiplier, axis; uint32_t alpha_bits; } yf_graph_op;",
           "static const yf_graph_op yf_graph_ops[YF_GRAPH_N_OPS] = {"]
    for o in ops:
        out.append("  {%d, {%d, %d, %d}, %d, %d, %d, %d, %d, %d, %d, %d, 0x%08xu}," % (
            o["op"], *o["ins"], o["out"], o["padding"], o["sw"], o["sh"], o["fw"], o["fh"], o["dm"], o["axis"], o["alpha_bits"]))
    out += ["};", "",
            "typedef struct { int32_t shape[4]; uint8_t type, is_const; int8_t qdim; uint16_t n_scales; } yf_graph_tensor;",
            f"static const yf_graph_tensor yf_graph_tensors[{len(T)}] = {{"]
    for t in T:
        out.append("  {{%d, %d, %d, %d}, %d, %d, %d, %d}," % (*t["shape"], t["type"], int(t["data"] is not None), t["qdim"], len(t["scale"])))
    pads = [i for i, o in enumerate(ops) if o["op"] == OPCODE["PAD"]]
    pad_t = {ops[i]["ins"][1] for i in pads}
    assert len(pad_t) == 1
    pt = pad_t.pop()
    out += ["};", "", f"/* the paddings of the PAD ops (tensor {pt}): top and left 1 */",
            f"#define YF_GRAPH_PAD_TENSOR {pt}",
            "static const int32_t yf_graph_paddings[%d] = {%s};" % (len(T[pt]["data"]), ", ".join(str(int(v)) for v in T[pt]["data"])),
            "", "#endif /* YF_GRAPH_GEN_H */", ""]
    return "\n".join(out)


# ---------------------------------------------------------------------------------------------------------------- .tflite reader
# builtin operator codes used by the model (schema.fbs BuiltinOperator)
BUILTIN = {0: "ADD", 2: "CONCATENATION", 3: "CONV_2D", 4: "DEPTHWISE_CONV_2D", 17: "MAX_POOL_2D",
           34: "PAD", 98: "LEAKY_RELU", 114: "QUANTIZE"}
TENSOR_TYPE = {0: "FLOAT32", 2: "INT32", 3: "UINT8", 4: "INT64", 9: "INT8"}
NP_TYPE = {"FLOAT32": np.float32, "INT32": np.int32, "UINT8": np.uint8, "INT64": np.int64, "INT8": np.int8}


class _FB:
    """Flatbuffer mechanics: tables, vtables, vectors, strings."""

    def __init__(self, buf):
        self.b = buf

    def u8(self, o): return self.b[o]
    def i8(self, o): return struct.unpack_from("<b", self.b, o)[0]
    def u16(self, o): return struct.unpack_from("<H", self.b, o)[0]
    def i32(self, o): return struct.unpack_from("<i", self.b, o)[0]
    def u32(self, o): return struct.unpack_from("<I", self.b, o)[0]
    def i64(self, o): return struct.unpack_from("<q", self.b, o)[0]
    def f32(self, o): return struct.unpack_from("<f", self.b, o)[0]

    def root(self):
        return self.u32(0)

    def field(self, table, slot):
        """Absolute offset of field `slot` of `table`, or None when absent (default)."""
        vt = table - self.i32(table)
        vt_len = self.u16(vt)
        pos = 4 + 2 * slot
        if pos >= vt_len:
            return None
        off = self.u16(vt + pos)
        return table + off if off else None

    def indirect(self, o):
        return o + self.u32(o)

    def vec(self, table, slot):
        """(start, length) of the vector in field `slot` or (None, 0)."""
        f = self.field(table, slot)
        if f is None:
            return None, 0
        v = self.indirect(f)
        return v + 4, self.u32(v)

    def table_vec(self, table, slot):
        s, n = self.vec(table, slot)
        return [self.indirect(s + 4 * i) for i in range(n)]

    def np_vec(self, table, slot, dtype):
        s, n = self.vec(table, slot)
        if s is None:
            return np.zeros(0, dtype)
        return np.frombuffer(self.b, dtype=dtype, count=n, offset=s).copy()

    def string(self, table, slot):
        s, n = self.vec(table, slot)
        return bytes(self.b[s:s + n]).decode("utf-8") if s is not None else ""

    def scalar(self, table, slot, kind, default=0):
        f = self.field(table, slot)
        if f is None:
            return default
        return getattr(self, kind)(f)


def read_tflite(path_or_bytes):
    """A .tflite file (path) or its bytes -> dict of tensors, ops, inputs, outputs."""
    buf = path_or_bytes if isinstance(path_or_bytes, (bytes, bytearray, memoryview)) else open(path_or_bytes, "rb").read()
    fb = _FB(buf)
    model = fb.root()
    version = fb.scalar(model, 0, "u32")
    opcodes = []
    for t in fb.table_vec(model, 1):
        dep = fb.scalar(t, 0, "i8")
        new = fb.scalar(t, 3, "i32")
        opcodes.append(max(dep, new))
    buffers = []
    for t in fb.table_vec(model, 4):
        s, n = fb.vec(t, 0)
        buffers.append(bytes(buf[s:s + n]) if s is not None else b"")
    subgraphs = fb.table_vec(model, 2)
    assert len(subgraphs) == 1
    sg = subgraphs[0]
    tensors = []
    for t in fb.table_vec(sg, 0):
        shape = fb.np_vec(t, 0, np.int32).tolist()
        ttype = TENSOR_TYPE[fb.scalar(t, 1, "u8")]
        bidx = fb.scalar(t, 2, "u32")
        name = fb.string(t, 3)
        q = fb.field(t, 4)
        scale = np.zeros(0, np.float32)
        zp = np.zeros(0, np.int64)
        qdim = 0
        if q is not None:
            qt = fb.indirect(q)
            scale = fb.np_vec(qt, 2, np.float32)
            zp = fb.np_vec(qt, 3, np.int64)
            qdim = fb.scalar(qt, 6, "i32")
        data = None
        if buffers[bidx]:
            data = np.frombuffer(buffers[bidx], dtype=NP_TYPE[ttype]).reshape(shape).copy()
        tensors.append(dict(name=name, shape=shape, type=ttype, buffer=bidx, scale=scale, zero_point=zp,
                            quantized_dimension=qdim, data=data))
    ops = []
    for t in fb.table_vec(sg, 3):
        code = opcodes[fb.scalar(t, 0, "u32")]
        name = BUILTIN[code]
        ins = fb.np_vec(t, 1, np.int32).tolist()
        outs = fb.np_vec(t, 2, np.int32).tolist()
        opt = fb.field(t, 4)
        o = {}
        if opt is not None:
            ot = fb.indirect(opt)
            if name == "CONV_2D":
                o = dict(padding=fb.scalar(ot, 0, "i8"), stride_w=fb.scalar(ot, 1, "i32"),
                         stride_h=fb.scalar(ot, 2, "i32"), fused_act=fb.scalar(ot, 3, "i8"),
                         dil_w=fb.scalar(ot, 4, "i32", 1), dil_h=fb.scalar(ot, 5, "i32", 1))
            elif name == "DEPTHWISE_CONV_2D":
                o = dict(padding=fb.scalar(ot, 0, "i8"), stride_w=fb.scalar(ot, 1, "i32"),
                         stride_h=fb.scalar(ot, 2, "i32"), depth_multiplier=fb.scalar(ot, 3, "i32"),
                         fused_act=fb.scalar(ot, 4, "i8"), dil_w=fb.scalar(ot, 5, "i32", 1),
                         dil_h=fb.scalar(ot, 6, "i32", 1))
            elif name == "MAX_POOL_2D":
                o = dict(padding=fb.scalar(ot, 0, "i8"), stride_w=fb.scalar(ot, 1, "i32"),
                         stride_h=fb.scalar(ot, 2, "i32"), filter_w=fb.scalar(ot, 3, "i32"),
                         filter_h=fb.scalar(ot, 4, "i32"), fused_act=fb.scalar(ot, 5, "i8"))
            elif name == "LEAKY_RELU":
                o = dict(alpha=fb.scalar(ot, 0, "f32"))
            elif name == "CONCATENATION":
                o = dict(axis=fb.scalar(ot, 0, "i32"), fused_act=fb.scalar(ot, 1, "i8"))
            elif name == "ADD":
                o = dict(fused_act=fb.scalar(ot, 0, "i8"))
        ops.append(dict(op=name, inputs=ins, outputs=outs, options=o))
    inputs = fb.np_vec(sg, 1, np.int32).tolist()
    outputs = fb.np_vec(sg, 2, np.int32).tolist()
    return dict(version=version, tensors=tensors, ops=ops, inputs=inputs, outputs=outputs,
                description=fb.string(model, 3))
