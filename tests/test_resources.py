"""Volume / Dict / Queue / Secret / Image / Sandbox semantics.

Reference behavior spec: diffusers_lora_finetune.py:343,367 (volume commit/
reload), dicts_and_queues.py:72-95, sandbox_pool.py:80-292 (queue partitions),
safe_code_execution.py:28-46 (sandbox exec)."""
import pytest

import modal_examples_amd as modal


def _require_mount_namespace():
    """Read-only bind mounts need a private mount namespace: CAP_SYS_ADMIN,
    or a kernel that lets this user create user namespaces.  Asked of the
    kernel in a throwaway child, before the test does any work."""
    import subprocess
    import sys

    probe = (
        "import ctypes, sys\n"
        "libc = ctypes.CDLL('libc.so.6', use_errno=True)\n"
        "ok = libc.unshare(0x00020000) == 0 or "
        "libc.unshare(0x10000000 | 0x00020000) == 0\n"
        "sys.exit(0 if ok else 1)\n")
    if subprocess.run([sys.executable, "-c", probe], timeout=60).returncode != 0:
        pytest.skip("needs a private mount namespace: this user has neither "
                    "CAP_SYS_ADMIN nor permission to create user namespaces "
                    "(user.max_user_namespaces is 0 or the kernel denies it)")


def test_volume_write_read_across_processes():
    vol = modal.Volume.from_name("test-vol", create_if_missing=True)
    app = modal.App("test-vol-app")

    @app.function()
    def writer(text):
        v = modal.Volume.from_name("test-vol")
        (v.path / "data.txt").write_text(text)
        v.commit()
        return str(v.path)

    writer.remote("hello-volume")
    vol.reload()
    assert vol.read_file("data.txt") == b"hello-volume"
    assert "data.txt" in vol.listdir("/")
    modal.Volume.delete("test-vol")


def test_volume_ephemeral():
    with modal.Volume.ephemeral() as v:
        (v.path / "x").write_text("1")
        assert v.listdir("/") == ["x"]


def test_dict_ops():
    with modal.Dict.ephemeral() as d:
        d["a"] = 1
        d.put("b", {"nested": [1, 2]})
        assert d["a"] == 1
        assert d.get("b")["nested"] == [1, 2]
        assert "a" in d
        assert len(d) == 2
        assert sorted(d.keys()) == ["a", "b"]
        assert d.pop("a") == 1
        assert len(d) == 1
        with pytest.raises(KeyError):
            d["missing"]


def test_dict_shared_across_workers():
    d = modal.Dict.from_name("test-shared-dict")
    d.clear()
    app = modal.App("test-dict-app")

    @app.function()
    def put(k, v):
        modal.Dict.from_name("test-shared-dict")[k] = v

    put.remote("from-worker", 42)
    assert d["from-worker"] == 42
    modal.Dict.delete("test-shared-dict")


def test_queue_fifo_and_partitions():
    with modal.Queue.ephemeral() as q:
        q.put(1)
        q.put_many([2, 3])
        q.put("p1", partition="other")
        assert q.get() == 1
        assert q.get_many(2) == [2, 3]
        assert q.len() == 0
        assert q.len(partition="other") == 1
        assert q.get(partition="other") == "p1"


def test_queue_get_nonblocking_empty():
    with modal.Queue.ephemeral() as q:
        assert q.get(block=False) is None
        assert q.get_many(3, block=False) == []


def test_secret_from_dict_injects_env():
    app = modal.App("test-secret-app")
    s = modal.Secret.from_dict({"MY_TEST_KEY": "sekrit"})

    @app.function(secrets=[s])
    def read_env():
        import os

        return os.environ.get("MY_TEST_KEY")

    assert read_env.remote() == "sekrit"


def test_secret_required_keys_missing():
    with pytest.raises(modal.NotFoundError):
        modal.Secret.from_name("nonexistent", required_keys=["NOPE_NOT_SET_XYZ"])


def test_image_chain_and_hash():
    img = (
        modal.Image.debian_slim(python_version="3.12")
        .apt_install("git")
        .uv_pip_install("torch")
        .env({"HELLO": "world"})
    )
    assert img.content_hash()
    assert img.build_env == {"HELLO": "world"}
    img2 = img.env({"X": "1"})
    assert img2.content_hash() != img.content_hash()


def test_image_imports_suppresses():
    img = modal.Image.debian_slim()
    with img.imports():
        import nonexistent_module_xyz  # noqa: F401


def test_sandbox_exec():
    sb = modal.Sandbox.create(app=None, timeout=30)
    p = sb.exec("echo", "hello-sandbox")
    assert p.wait() == 0
    assert "hello-sandbox" in p.stdout.read()
    sb.terminate()


def test_sandbox_entrypoint_and_poll():
    sb = modal.Sandbox.create("python3", "-c", "print(6*7)", timeout=30)
    assert sb.wait() == 0
    assert "42" in sb.stdout.read()
    sb.terminate()


def test_cron_matching():
    c = modal.Cron("*/5 14 * * *")
    import time as _t

    t = _t.struct_time((2026, 9, 11, 14, 10, 0, 4, 254, 0))
    assert c.matches(t)
    t2 = _t.struct_time((2026, 9, 11, 15, 10, 0, 4, 254, 0))
    assert not c.matches(t2)


def test_period_validation():
    assert modal.Period(minutes=5).total_seconds == 300
    with pytest.raises(modal.InvalidError):
        modal.Period()


def test_gpu_string_parsing():
    from modal_examples_amd.gpu.device_pool import parse_gpu

    assert parse_gpu(None) == 0
    assert parse_gpu("mi355x") == 1
    assert parse_gpu("MI355X:4") == 4
    assert parse_gpu("H100!") == 1
    assert parse_gpu(["H100:2", "A100"]) == 2


def test_volume_mount_path_in_worker():
    """volumes={'/mnt/x': vol} symlinks the mount path inside the worker."""
    vol = modal.Volume.from_name("mount-test-vol", create_if_missing=True)
    (vol.path / "probe.txt").write_text("mounted!")
    app = modal.App("test-mount-app")

    @app.function(volumes={"/tmp/mxa_mount_test": vol})
    def read_mounted():
        with open("/tmp/mxa_mount_test/probe.txt") as f:
            return f.read()

    assert read_mounted.remote() == "mounted!"
    modal.Volume.delete("mount-test-vol")
    import os

    if os.path.islink("/tmp/mxa_mount_test"):
        os.unlink("/tmp/mxa_mount_test")


def test_image_env_reaches_worker():
    img = modal.Image.debian_slim().env({"IMG_LAYER_VAR": "layered"})
    app = modal.App("test-imgenv-app")

    @app.function(image=img)
    def read_env():
        import os

        return os.environ.get("IMG_LAYER_VAR")

    assert read_env.remote() == "layered"


def test_volume_read_only_api():
    """Volume.read_only(): write APIs raise, reads still work."""
    vol = modal.Volume.from_name("ro-api-vol", create_if_missing=True)
    (vol.path / "d.txt").write_text("ro")
    ro = vol.read_only()
    assert ro.read_file("d.txt") == b"ro"
    assert "d.txt" in ro.listdir("/")
    from modal_examples_amd.exception import InvalidError

    with pytest.raises(InvalidError):
        ro.commit()
    with pytest.raises(InvalidError):
        ro.remove_file("d.txt")
    with pytest.raises(InvalidError):
        ro.batch_upload()
    assert ro.read_only() is ro
    modal.Volume.delete("ro-api-vol")


def test_volume_read_only_mount_enforced_in_worker():
    """A read-only mount is a ro bind mount in the worker's private mount
    namespace: raw file writes fail with EROFS, reads work, and the parent
    namespace (this process) never sees the mount."""
    _require_mount_namespace()
    vol = modal.Volume.from_name("ro-mount-vol", create_if_missing=True)
    (vol.path / "probe.txt").write_text("ro-mounted")
    app = modal.App("test-ro-mount-app")
    mnt = "/tmp/mxa_ro_mount_test"

    @app.function(volumes={mnt: vol.read_only()})
    def probe():
        import errno

        with open(f"{mnt}/probe.txt") as f:
            content = f.read()
        try:
            open(f"{mnt}/new.txt", "w")
            write = "allowed"
        except OSError as e:
            write = "EROFS" if e.errno == errno.EROFS else f"errno={e.errno}"
        return content, write

    content, write = probe.remote()
    assert content == "ro-mounted"
    assert write == "EROFS"
    # volume itself untouched and still writable from here
    assert not (vol.path / "new.txt").exists()
    (vol.path / "after.txt").write_text("ok")
    modal.Volume.delete("ro-mount-vol")
    import os
    import shutil

    if os.path.isdir(mnt) and not os.path.islink(mnt):
        shutil.rmtree(mnt, ignore_errors=True)


def test_image_run_function_runs_in_worker():
    """Image.run_function build steps execute in a worker process (with the
    requested volumes), not in the client (reference: build-time weight
    downloads run inside a container)."""
    import os

    vol = modal.Volume.from_name("img-build-vol", create_if_missing=True)

    def download_weights():
        v = modal.Volume.from_name("img-build-vol")
        (v.path / "weights.bin").write_bytes(b"W" * 16)
        (v.path / "pid.txt").write_text(str(os.getpid()))
        v.commit()

    img = modal.Image.debian_slim().run_function(
        download_weights, volumes={"/tmp/mxa_imgbuild_vol": vol})
    app = modal.App("test-img-build", image=img)

    @app.function()
    def use_weights():
        v = modal.Volume.from_name("img-build-vol")
        return v.read_file("weights.bin")

    assert use_weights.remote() == b"W" * 16
    # the build step ran in a different process than this client
    assert (vol.path / "pid.txt").read_text() != str(os.getpid())
    modal.Volume.delete("img-build-vol")
    if os.path.islink("/tmp/mxa_imgbuild_vol"):
        os.unlink("/tmp/mxa_imgbuild_vol")


def test_sandbox_from_id_cross_process():
    """A sandbox created in one process can be attached from ANOTHER via the
    store-backed registry: exec in its workdir, poll, terminate."""
    import subprocess
    import sys
    import textwrap
    from pathlib import Path

    sb = modal.Sandbox.create("sleep", "30")
    (Path(sb.workdir) / "marker.txt").write_text("shared")
    probe = textwrap.dedent(f"""
        import modal_examples_amd as modal
        h = modal.Sandbox.from_id({sb.object_id!r})
        assert h.poll() is None          # still running
        p = h.exec("cat", "marker.txt")  # runs in the sandbox workdir
        assert p.wait() == 0
        print("READ:" + p.stdout.read().strip())
        h.terminate()
    """)
    repo = str(Path(__file__).resolve().parent.parent)
    r = subprocess.run([sys.executable, "-c", probe], capture_output=True,
                       text=True, cwd=repo, timeout=60)
    assert r.returncode == 0, r.stderr[-1500:]
    assert "READ:shared" in r.stdout
    import time as _time

    for _ in range(50):  # the other process killed the main proc
        if sb.poll() is not None:
            break
        _time.sleep(0.1)
    assert sb.poll() is not None


def test_period_schedule_fires_live():
    """A deployed Period(seconds=...) schedule actually invokes the function
    repeatedly (live end of runtime/cron.py, beyond the matching logic)."""
    import time

    app_s = modal.App("test-live-schedule")
    counter = modal.Dict.from_name("sched-count", create_if_missing=True)
    counter.clear()
    counter["n"] = 0

    @app_s.function(schedule=modal.Period(seconds=0.3))
    def tick():
        d = modal.Dict.from_name("sched-count")
        d["n"] = d.get("n", 0) + 1

    app_s.deploy()
    deadline = time.time() + 20
    while counter.get("n", 0) < 2 and time.time() < deadline:
        time.sleep(0.1)
    assert counter.get("n", 0) >= 2, "schedule did not fire repeatedly"
    from modal_examples_amd.runtime.cron import stop_schedules

    stop_schedules("test-live-schedule")
    modal.Dict.delete("sched-count")


def test_bucket_mount_read_only():
    """CloudBucketMount(read_only=True) gets the same filesystem-level
    enforcement as Volume.read_only() (ro bind mount in the worker)."""
    _require_mount_namespace()
    bucket =modal.CloudBucketMount("models-bucket", read_only=True)
    # pre-populate the local bucket dir
    (bucket.path / "weights.txt").write_text("frozen")
    app_b = modal.App("test-bucket-ro")
    mnt = "/tmp/mxa_bucket_ro_test"

    @app_b.function(volumes={mnt: bucket})
    def probe():
        import errno

        with open(f"{mnt}/weights.txt") as f:
            content = f.read()
        try:
            open(f"{mnt}/new.txt", "w")
            blocked = False
        except OSError as e:
            blocked = e.errno == errno.EROFS
        return content, blocked

    content, blocked = probe.remote()
    assert content == "frozen"
    assert blocked
    import os
    import shutil

    if os.path.isdir(mnt) and not os.path.islink(mnt):
        shutil.rmtree(mnt, ignore_errors=True)


def test_volume_from_name_missing_raises():
    """from_name(create_if_missing=False) on a nonexistent volume raises
    NotFoundError instead of silently creating it (ADVICE r1 finding)."""
    import pytest as _pytest

    with _pytest.raises(modal.NotFoundError):
        modal.Volume.from_name("never-created-vol-xyz")


def test_image_pip_layers_build_isolated_venv():
    """pip layers materialize a content-hashed venv and the worker runs under
    its interpreter (sys.prefix is the venv), not a bare importability check
    (r1 VERDICT missing #7)."""
    app = modal.App("test-image-venv")
    img = modal.Image.debian_slim().uv_pip_install("numpy")

    @app.function(image=img)
    def which_python() -> dict:
        import sys

        import numpy

        return {"prefix": sys.prefix, "exe": sys.executable,
                "numpy": numpy.__version__}

    out = which_python.remote()
    assert img.content_hash() in out["prefix"], out
    assert out["prefix"] != __import__("sys").base_prefix


def test_image_unsatisfiable_pip_layer_fails_loudly():
    app = modal.App("test-image-badpip")
    img = modal.Image.debian_slim().pip_install("definitely-not-a-real-pkg-xyz-123")

    @app.function(image=img)
    def f():
        return 1

    with pytest.raises(Exception, match="cannot be satisfied offline"):
        f.remote()


def test_s3_endpoint_roundtrip():
    """Local S3-compatible endpoint: PUT/GET/LIST/DELETE over real HTTP."""
    from modal_examples_amd.resources.s3local import S3Client, start_s3_server

    c = S3Client(start_s3_server())
    c.put("t-bucket", "a/x.txt", b"hello")
    c.put("t-bucket", "a/y.txt", b"world")
    c.put("t-bucket", "b/z.txt", b"nope")
    assert sorted(c.list("t-bucket", "a/")) == ["a/x.txt", "a/y.txt"]
    assert c.get("t-bucket", "a/x.txt") == b"hello"
    c.delete("t-bucket", "a/y.txt")
    assert c.list("t-bucket", "a/") == ["a/x.txt"]


def test_bucket_mount_prefix_sync_and_writeback(tmp_path):
    """CloudBucketMount: worker sees a PRIVATE synced copy of the bucket
    prefix (downloaded over the S3 endpoint, not a shared symlink) and its
    writes land back in the bucket at worker exit."""
    import time

    from modal_examples_amd.resources.s3local import S3Client, start_s3_server

    ep = start_s3_server()
    c = S3Client(ep)
    c.put("sync-bkt", "data/in.txt", b"seeded")
    c.put("sync-bkt", "other/skip.txt", b"outside prefix")

    app = modal.App("test-s3-mount")
    mnt = modal.CloudBucketMount("sync-bkt", key_prefix="data")

    # a mount point any user can create, unlike one under /mnt
    mount_path = str(tmp_path / "bkt")

    @app.function(volumes={mount_path: mnt}, scaledown_window=0.5)
    def roundtrip() -> dict:
        import os
        from pathlib import Path

        p = Path(mount_path)
        seen = sorted(f.name for f in p.glob("**/*") if f.is_file())
        (p / "out.txt").write_text("produced")
        real = os.path.realpath(p)
        return {"seen": seen, "private": "s3mount" in real}

    out = roundtrip.remote()
    assert out["seen"] == ["in.txt"], out
    assert out["private"], out  # synced copy, not the server-side dir
    # writeback happens at worker shutdown (scaledown reaps the idle worker)
    deadline = time.monotonic() + 20
    while time.monotonic() < deadline:
        if "data/out.txt" in c.list("sync-bkt", "data/"):
            break
        time.sleep(0.3)
    assert c.get("sync-bkt", "data/out.txt") == b"produced"


def test_sandbox_wait_until_ready_and_detach(tmp_path):
    marker = tmp_path / "ready"
    sb = modal.Sandbox.create(
        "bash", "-c", f"sleep 0.7; touch {marker}; sleep 30",
        timeout=60,
        readiness_probe=modal.Probe.with_exec(["test", "-f", str(marker)]))
    try:
        assert sb.wait_until_ready(20) is True
        assert sb.poll() is None  # still running
        assert sb.detach() is sb
        sb2 = modal.Sandbox.from_id(sb.object_id)
        assert sb2.poll() is None
    finally:
        sb.terminate()


def test_s3_endpoint_rejects_path_traversal():
    import urllib.error
    import urllib.request

    from modal_examples_amd.resources.s3local import S3Client, start_s3_server

    ep = start_s3_server()
    c = S3Client(ep)
    c.put("trav-bkt", "safe.txt", b"ok")
    for bad in ("trav-bkt/../../escape.txt", "..%2F..%2Fescape"):
        req = urllib.request.Request(f"{ep}/{bad}", data=b"x", method="PUT")
        try:
            urllib.request.urlopen(req, timeout=5)
            raised = False
        except urllib.error.HTTPError as e:
            raised = e.code == 400
        assert raised, bad
    assert c.get("trav-bkt", "safe.txt") == b"ok"
