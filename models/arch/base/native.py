"""Module side of the native narrow-band paths (NBC2, NBC, NB-BLSTM -> nbss_amd/nbc2.py, nbc.py, blstm.py): the runner of a module, and the one warning
that names why a call on a HIP device took the torch.nn modules instead."""
import importlib
import warnings
import weakref

# module -> (its nbss_amd runner or None, the reason it is None).  Module level and weakly keyed: a ctypes library handle as an attribute of the module
# would break deepcopy / pickle of the module, and the entry goes when the module does (the runner itself holds its module weakly).
NATIVE = weakref.WeakKeyDictionary()
_NOTED = weakref.WeakKeyDictionary()  # module -> reasons already reported


def native_runner(module, where: str, cls: str):
    """(runner, None) when the HIP library is there and `module` is a configuration the kernels of `where`.`cls` (e.g. "nbss_amd.nbc2", "NativeNBC2") are
    built for, else (None, reason); decided once per module.  A library that cannot be loaded means the torch.nn path, not an exception: its text is the
    reason, which forward() reports once."""
    if module not in NATIVE:
        runner, why = None, None
        try:
            from nbss_amd._lib import hip
            runner_cls = getattr(importlib.import_module(where), cls)
            why = runner_cls.supported(module)
            if why is None:
                runner = runner_cls(module, hip())
        except Exception as e:  # (no library / no HIP runtime: torch.nn)
            runner, why = None, f"{type(e).__name__}: {e}"
        NATIVE[module] = (runner, why)
    return NATIVE[module]


def torch_path_note(module, label: str, why: str, stacklevel: int = 3) -> None:
    """one warning per module and reason: a user on a HIP device can tell which path ran.  To be called from the module's forward(): the warning points
    at the frame that called forward() (a helper between forward() and this call adds one to `stacklevel`)."""
    seen = _NOTED.setdefault(module, set())
    if why not in seen:
        seen.add(why)
        warnings.warn(f"{label}: torch.nn path instead of the native HIP kernels ({why})", RuntimeWarning, stacklevel=stacklevel)
