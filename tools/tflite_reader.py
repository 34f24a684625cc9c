"""The minimal TFLite flatbuffer reader moved into the package (stm32h7-yolo_amd/model_file.py, which also converts a .tflite to the
.yfm pack); this name stays for the dev tools that import it.
"""
import importlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
read_tflite = importlib.import_module("stm32h7-yolo_amd.model_file").read_tflite

if __name__ == "__main__":
    m = read_tflite(sys.argv[1])
    print("version", m["version"], "tensors", len(m["tensors"]), "ops", len(m["ops"]), "in", m["inputs"], "out", m["outputs"])
    for i, op in enumerate(m["ops"]):
        print(i, op["op"], op["inputs"], op["outputs"], op["options"])
