"""Host-side checks that need no GPU: the C-ABI library exists and exports exactly what include/lbc_hip.h declares,
the product loader has no fallback, and the drop-in modules reproduce the reference's state_dict layout."""
import ctypes
import json
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


def declared_functions():
    src = open(os.path.join(ROOT, "include", "lbc_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(lbc_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_declared_symbol():
    from learningbycheating_amd import _lib
    assert os.path.exists(_lib.LIB_PATH), "run __graft_entry__.build() first"
    lib = ctypes.CDLL(_lib.LIB_PATH)          # loading needs no GPU; no compute call is made here
    names = declared_functions()
    assert len(names) >= 24
    for n in names:
        assert hasattr(lib, n), "liblbc_hip.so does not export %s" % n
    lib.lbc_backend.restype = ctypes.c_char_p
    assert lib.lbc_backend().decode() == "hip-gfx950"
    assert set(_lib.EXPORTED_SYMBOLS) <= set(names) | {"lbc_profile_enable", "lbc_profile_report"}


def test_loader_fails_loudly_without_library(tmp_path):
    from learningbycheating_amd import _lib
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _lib.load(str(tmp_path / "missing.so"))


def test_cpu_tensors_are_rejected_by_the_product_path():
    from learningbycheating_amd import _lib
    from learningbycheating_amd.bird_view.models import ImagePolicyModelSS
    _lib._inject_for_tests(None)
    _lib.load()
    net = ImagePolicyModelSS("resnet18")
    with pytest.raises(RuntimeError, match="no CPU path"):
        net(torch.zeros(1, 3, 160, 384), torch.zeros(1), torch.zeros(1, 4))


def test_module_state_dict_layout_equals_reference():
    from learningbycheating_amd.bird_view.models import ImagePolicyModelSS, BirdViewPolicyModelSS
    lay = json.load(open(os.path.join(GOLD, "state_dict_layout.json")))
    for name, net in (("image_resnet34", ImagePolicyModelSS("resnet34")), ("birdview_resnet18", BirdViewPolicyModelSS("resnet18"))):
        got = [(k, list(v.shape), str(v.dtype)) for k, v in net.state_dict().items()]
        assert got == [tuple(x) if False else (x[0], x[1], x[2]) for x in lay[name]]
    # ctor contract (reference image.py:23 / birdview.py:48; benchmark_agent.py:34 passes model=, backbone=, imagenet_pretrained=)
    n = ImagePolicyModelSS(**{"model": "image_ss", "backbone": "resnet34", "imagenet_pretrained": False})
    assert n.all_branch is False and hasattr(n, "conv") and hasattr(n, "deconv") and hasattr(n, "location_pred")
    assert ImagePolicyModelSS("resnet34", all_branch=True).all_branch is True
    with pytest.raises(NotImplementedError):
        ImagePolicyModelSS("resnet34", warp=True)


def test_weights_are_channels_last_and_survive_load_and_to():
    from learningbycheating_amd.bird_view.models import BirdViewPolicyModelSS
    from learningbycheating_amd.engine import is_channels_last_4d
    from oracle import lbc_oracle as O
    net = BirdViewPolicyModelSS("resnet18")
    sd = O.make_state_dict("birdview", "resnet18", 9)
    net.load_state_dict(sd, strict=True)
    net = net.to(torch.float32)
    for k, p in net.named_parameters():
        assert is_channels_last_4d(p.data), k
        assert torch.equal(p.data, sd[k]), k            # logical values/shapes unchanged
    out = net.state_dict()
    assert list(out.keys()) == list(sd.keys())


def _recorded_reference_module(layout):
    """a module whose state_dict holds exactly the (key, shape, dtype) entries the REAL reference class had when oracle/make_golden.py
    recorded tests/golden/state_dict_layout.json: a strict load_state_dict into it checks what the reference class's strict load checks
    (the key set and every shape), and what it saves has the reference checkpoint's keys, shapes and dtypes"""
    root = torch.nn.Module()
    for key, shape, dt in layout:
        *path, leaf = key.split(".")
        m = root
        for p in path:
            if p not in m._modules:
                m.add_module(p, torch.nn.Module())
            m = m._modules[p]
        m.register_buffer(leaf, torch.zeros(shape, dtype=getattr(torch, dt.split(".", 1)[1])))
    return root


def test_checkpoint_round_trip_with_reference_classes(tmp_path):
    """our .th -> reference class (strict) and reference .th -> ours, through the logic of benchmark_agent.py:27-38; the reference
    class is stood in for by its recorded state_dict layout (tests/golden), so the check runs wherever the suite runs"""
    from learningbycheating_amd.bird_view.models import ImagePolicyModelSS, BirdViewPolicyModelSS
    from oracle import lbc_oracle as O
    lay = json.load(open(os.path.join(GOLD, "state_dict_layout.json")))
    for kind, backbone, ours in (("image", "resnet34", ImagePolicyModelSS), ("birdview", "resnet18", BirdViewPolicyModelSS)):
        mine = ours(backbone)
        mine.load_state_dict(O.make_state_dict(kind, backbone, 17))
        path = tmp_path / ("model-%s.th" % kind)
        torch.save(mine.state_dict(), str(path))
        config = {"model_args": {"model": "image_ss" if kind == "image" else "birdview_dian", "backbone": backbone, "imagenet_pretrained": False}}
        recorded = lay["%s_%s" % (kind, backbone)]
        ref = _recorded_reference_module(recorded)
        saved = torch.load(str(path))
        assert {k: str(v.dtype) for k, v in saved.items()} == {k: dt for k, _, dt in recorded}
        ref.load_state_dict(saved)          # strict, as benchmark_agent.py:37
        ref.eval()
        for k, v in ref.state_dict().items():
            assert torch.equal(v, mine.state_dict()[k]), k
        # a checkpoint written by the reference class: other values, the recorded keys / shapes / dtypes
        ref.load_state_dict(O.make_state_dict(kind, backbone, 18))
        path2 = tmp_path / ("ref-%s.th" % kind)
        torch.save(ref.state_dict(), str(path2))
        again = ours(**config["model_args"])
        again.load_state_dict(torch.load(str(path2)))
        for k, v in again.state_dict().items():
            assert torch.equal(v, ref.state_dict()[k]), k


def test_comm_entry_points_validate_without_a_gpu():
    """lbc_comm_* (the RCCL communicator of synchronized BatchNorm): RCCL is bound at run time, so without it the calls fail
    with a message instead of the library failing to load; argument errors are reported before RCCL is touched"""
    import ctypes
    from learningbycheating_amd import _lib
    lib = _lib.get()
    ident = torch.zeros(128, dtype=torch.uint8)
    rc = lib.lbc_comm_unique_id(_lib.ptr(ident))
    if rc == 0:
        assert int(ident.count_nonzero()) > 0
    else:
        assert b"rccl" in lib.lbc_last_error().lower()
    comm = ctypes.c_void_p()
    assert lib.lbc_comm_create(_lib.ptr(ident), 2, 2, ctypes.byref(comm)) != 0 and b"rank 2 outside" in lib.lbc_last_error()
    assert lib.lbc_comm_create(None, 0, 1, ctypes.byref(comm)) != 0
    assert lib.lbc_comm_allreduce_f32(None, None, 4, None) != 0
    assert lib.lbc_comm_world_size(None) == 0
    lib.lbc_comm_destroy(None)
    # the executor refuses a hook without its scratch row
    from learningbycheating_amd.engine import PolicyEngine
    eng = PolicyEngine(18, 3, 32, 64, True, 1, torch.device("cpu"))
    fn = ctypes.cast(lib.lbc_comm_allreduce_f32, ctypes.c_void_p)
    assert lib.lbc_net_set_sync_bn(eng.handle, fn, None, 2, None, 0) != 0 and b"1536" in lib.lbc_last_error()
    assert lib.lbc_net_set_sync_bn(eng.handle, None, None, 1, None, 0) == 0


def test_c99_host_plans_the_network_through_the_header(tmp_path):
    """include/lbc_hip.h is C (not only C++): gcc -std=c99 -pedantic compiles it, and a C host that dlopens the product
    library plans ResNet-34 and reads the reference's state_dict names / parameter count from the tensor table"""
    import subprocess
    from learningbycheating_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    inc = os.path.join(root, "include")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-x", "c", os.path.join(inc, "lbc_hip.h")])
    exe = str(tmp_path / "host")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-I", inc, os.path.join(root, "tests", "c_host", "host.c"), "-o", exe, "-ldl"])
    out = subprocess.check_output([exe, _lib.LIB_PATH], timeout=120).decode()
    kv = dict(t.split("=", 1) for t in out.split())
    from learningbycheating_amd.bird_view.models import ImagePolicyModelSS
    net = ImagePolicyModelSS("resnet34", all_branch=True)
    sd = net.state_dict()
    assert kv["backend"] == "hip-gfx950"
    # (the unused ImageNet classifier `conv.fc.*` of the reference's torchvision trunk is in the state_dict, not in the plan)
    used = {k: v for k, v in sd.items() if not k.startswith("conv.fc.")}
    pused = [p for n, p in net.named_parameters() if not n.startswith("conv.fc.")]
    assert int(kv["tensors"]) == len(used) and kv["first"] in used and kv["last"] in used
    assert int(kv["params"]) == len(pused)
    assert int(kv["param_elems"]) == sum(p.numel() for p in pused)
    assert int(kv["workspace"]) > 0 and int(kv["stages"]) == 6


def test_descriptor_size_range_and_unknown_option_warning():
    """lbc_conv_desc.struct_size is accepted from the ABI-200 layout up to the library's own sizeof (fields appended later stay optional
    for older hosts), refused outside that range (too small, larger than the library knows) with a message that names the field; and an LBC_*
    environment variable that is not an option is reported on stderr when the library loads instead of being ignored silently."""
    import subprocess
    import sys
    from learningbycheating_amd import _lib
    lib = _lib.get()
    lib.lbc_conv2d_wgrad_workspace.restype = ctypes.c_size_t
    d = _lib.ConvDesc(2, 8, 8, 64, 64, 3, 3, 1, 1, 0, 0, 0)
    size = d.struct_size
    assert size == ctypes.sizeof(d) and lib.lbc_conv2d_wgrad_workspace(ctypes.byref(d)) > 0
    for bad in (0, size - 8, size + 8):
        d.struct_size = bad
        assert lib.lbc_conv2d_wgrad_workspace(ctypes.byref(d)) == 0 and b"struct_size" in lib.lbc_last_error(), bad
    d.struct_size = size
    assert lib.lbc_conv2d_wgrad_workspace(ctypes.byref(d)) > 0
    code = "from learningbycheating_amd import _lib; _lib.get().lbc_config_get(b'LBC_NO_HDMA')"
    env = dict(os.environ, LBC_HDMAP_PRE="1", LBC_NO_HDMA="0", LBC_TEST_VERBOSE="1", PYTHONPATH=ROOT)
    p = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, cwd=ROOT)
    assert p.returncode == 0, p.stderr
    assert "LBC_HDMAP_PRE is not an option" in p.stderr and "LBC_NO_HDMA is" not in p.stderr and "LBC_TEST_VERBOSE" not in p.stderr, p.stderr


def test_bank_conflict_model_of_the_border_select():
    """scripts/probe/lds_conflict_model.py (MI355X_MICROARCH.md LDS section: ds_read_b128 is served in four fixed 16-lane groups over 64 banks):
    the shared zero slot of conv_hdmap_k's border select costs +25 % LDS cycles on the A-fragment reads at W = 24 and +44 % at W = 12 -- what the PMC
    passes of rounds 3-5 measured as 13 % / 30 % of all LDS cycles -- and the lane's-own-bank zero costs none (measured on the GPU: 1.1 % / 0.9 %,
    and 0.5 % MORE step time under the power cap, which is why the library keeps the broadcast: profiles/r06_call1_*, r06_call15_*)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("lds_conflict_model", os.path.join(ROOT, "scripts", "probe", "lds_conflict_model.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    assert abs(m.sweep(24, 10, 256, 320, 0) - 0.25) < 0.01 and abs(m.sweep(12, 5, 128, 192, 0) - 0.444) < 0.01
    assert m.sweep(24, 10, 256, 320, 1) == 0.0 and m.sweep(12, 5, 128, 192, 1) == 0.0 and m.sweep(48, 20, 256, 384, 1) == 0.0
