"""CPU-side checks of the drop-in boundary: the C-ABI library loads and exports every symbol that
include/se_engine.h declares; no compute is attempted without a GPU."""
import ctypes
import os
import re

import pytest

from conftest import ROOT


def _declared():
    text = open(os.path.join(ROOT, "include", "se_engine.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b((?:se|fsn)_[a-z0-9_]+)\s*\(", text)))


def test_header_symbols_exported():
    from speech_enhancement_mi_amd import engine
    names = _declared()
    assert "se_step" in names and "se_realtime_process" in names and "fsn_realtime_process" in names and len(names) >= 25
    lib = ctypes.CDLL(engine.LIB_PATH)
    for n in names:
        assert hasattr(lib, n), f"{n} declared in se_engine.h but not exported by libse_engine.so"
    assert sorted(engine.EXPORTS) == names
    assert lib.se_abi_version() == 5


def _table():
    from speech_enhancement_mi_amd import engine
    return engine.prototypes(open(os.path.join(ROOT, "include", "se_engine.h")).read())


def test_derived_prototypes_one_function_per_scalar_kind():
    """engine.prototypes reads the ctypes table out of the header; written out here: a double in the middle, two floats, a uint32_t,
    char * outputs, an int64_t return, a const char * return, void."""
    from ctypes import c_char_p, c_double, c_float, c_int, c_int64, c_uint32, c_void_p as vp
    table = _table()
    assert table["se_hifi_seqnorm"] == (c_int, [vp] * 4 + [c_double] + [vp] * 3 + [c_int] * 5 + [vp])
    assert table["se_synth_rir"] == (c_int, [vp] * 4 + [c_int] * 6 + [c_float, c_float, c_int, vp, vp])
    assert table["se_synth_rir_tail"] == (c_int, [vp, vp, vp, c_int, c_int, c_int, c_int, c_float, c_uint32, vp])
    assert table["se_profile_read"] == (c_int, [vp, c_int, c_char_p, c_char_p, c_int, vp, vp, vp])
    assert table["fsn_train_ws_bytes_chains"] == (c_int64, [vp, c_int, c_int64, vp, vp])
    assert table["se_last_error"] == (c_char_p, [vp])
    assert table["se_destroy"] == (None, [vp])


def test_every_declared_function_has_a_prototype():
    """Two separate parses of the header (_declared above, the binding's) name the same functions, and load_library() has applied the
    binding's table to the library."""
    from speech_enhancement_mi_amd import engine
    table = _table()
    assert sorted(table) == _declared() == engine.EXPORTS
    lib = engine.load_library()
    for name, (restype, argtypes) in table.items():
        assert (getattr(lib, name).restype, list(getattr(lib, name).argtypes)) == (restype, argtypes), name


def test_prototypes_raise_on_a_type_they_do_not_know():
    from speech_enhancement_mi_amd import engine
    for line in ("int se_new(unsigned n);", "int se_new(size_t n, void *stream);", "long se_new(void);", "int se_new(float x[4]);",
                 "int se_new(se_config cfg);", "int se_new(int (*cb)(int));"):
        with pytest.raises(ValueError):
            engine.prototypes("int se_abi_version(void);\n" + line)
    # comments are no declarations
    assert engine.prototypes("/* int se_old(size_t n); */\nint se_abi_version(void);  // int se_older(long n);\n") == {"se_abi_version": (ctypes.c_int, [])}


def test_no_cpu_fallback():
    """Without a GPU the engine must fail loudly, never compute on the host."""
    import torch
    from speech_enhancement_mi_amd import engine
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    cfg = engine.make_config([4, 8, 8, 8], 201, 16, 3200, num_layers=2)
    with pytest.raises(RuntimeError, match="no HIP device|no CPU fallback|se_create failed"):
        engine.Engine(cfg)


def test_config_struct_sizes():
    """INTEGRATION.md's ctypes mirror of se_config must have the library's size (a short struct would leave `precision`
    reading whatever follows it): the library exports its own sizeof for the binding to check."""
    from speech_enhancement_mi_amd import engine
    lib = ctypes.CDLL(engine.LIB_PATH)
    assert lib.se_config_size() == ctypes.sizeof(engine.SeConfig)
    assert lib.fsn_config_size() == ctypes.sizeof(engine.FsnConfig)
    # the stub printed in INTEGRATION.md lists the same fields
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name, _ in engine.SeConfig._fields_:
        assert f'"{name}"' in text, f"INTEGRATION.md SeConfig stub lacks field {name}"
