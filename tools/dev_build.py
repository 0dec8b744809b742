"""Is libconan_hip.so a `make -C conan_amd/csrc DEV=1` build?  python tools/dev_build.py: exit status 0 when it is; otherwise says so and exits
with 1.  The library has no query for it: a stream-set is created with a DEV-only switch name (csrc/plan_switches.h), which the shipped
library rejects as unknown."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from conan_amd import _lib, configs, synth  # noqa: E402
from conan_amd.runtime import Context  # noqa: E402


def is_dev_build(ctx):
    try:
        ctx.streams(1, dev_plan="MEGA_LAYOUT=g").close()
    except _lib.ConanError as e:
        if e.code == _lib.ERR_INVALID and "unknown switch" in str(e):
            return False
        raise
    return True


def require_dev_build(ctx, what):
    if not is_dev_build(ctx):
        sys.exit(f"{what}: libconan_hip.so is not a DEV build - the shipped library has no MEGA_LAYOUT switch (a GPU memory fault under MEGA_LAYOUT=m is on "
                 "record, profiles/r6_stress_layout.txt).  Build with `make -C conan_amd/csrc DEV=1`; nothing was run.")


if __name__ == "__main__":
    chp = configs.conan_hparams()
    ctx = Context(chp, None, 0, False, True, False)
    ctx.load_state_dict("conan", synth.conan_state_dict(chp, 0))
    ctx.finalize()
    require_dev_build(ctx, "tools/dev_build.py")
    print("libconan_hip.so is a DEV build")
