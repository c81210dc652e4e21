"""A/B helper: run a script with bev_native loading another build of the library.
usage: python tools/with_lib.py <libbev.so> <script.py> [args...]
A build with another ABI number is loaded with a warning: an A/B across a bump is only sound where no signature
that the script uses changed, which is the caller's to know."""
import ctypes
import os
import runpy
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "vision-based-spatio-temporal-analysis_amd"))
import bev_native  # noqa: E402

bev_native.LIB_PATH = os.path.abspath(sys.argv[1])
_abi = ctypes.CDLL(bev_native.LIB_PATH).bev_abi_version()
if _abi != bev_native.ABI_VERSION:
    print(f"with_lib: {sys.argv[1]} has ABI {_abi}, this tree's bev_native expects {bev_native.ABI_VERSION}: loading it "
          "anyway; entry points whose signature changed in between must not be called", file=sys.stderr)
    bev_native.ABI_VERSION = _abi
script = sys.argv[2]
sys.argv = sys.argv[2:]
sys.path.insert(0, os.path.dirname(os.path.abspath(script)))
runpy.run_path(script, run_name="__main__")
