"""The package's loader (stm32h7-yolo_amd/libs.py) for the test modules: every host build they open, every make they start, under its build lock."""
import importlib

libs = importlib.import_module("stm32h7-yolo_amd.libs")
host_library = libs.host_library
