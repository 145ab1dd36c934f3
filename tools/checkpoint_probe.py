"""What a checkpoint of a frame costs (pt_frame_checkpoint_save / _load; include/pt_checkpoint.h), on one MI355X.

    python tools/checkpoint_probe.py [--workload dragon] [--width 1920] [--height 1080] [--quantum 8] [--adaptive-passes 6] [--out profiles/checkpoint_probe.json]

Two states of a 1920 x 1080 progressive frame: after one pass at a fixed sample count (every stream has a record, none has candidates),
and adaptive after several passes (records with candidates, finished pixels).  For each: the blob's size against the frame's park records
(528 bytes each), the time of a save (the size query, then the save: two packs) and of the save alone into a buffer of the right size,
the time of a load onto a second scene, and -- the yardstick, in the same run -- the time of a plain device-to-host copy of as many bytes
as the untrimmed park records take, into pageable memory as the blob is.  A checkpoint cannot beat that copy by much more than the ratio
of the sizes.  Every time is the best of --repeats."""
import argparse, ctypes as C, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import bench
from cpupathtrace_amd import binding, scenes


def best(fn, repeats):
    times = []
    for _ in range(repeats):
        t = time.perf_counter()
        out = fn()
        times.append((time.perf_counter() - t) * 1e3)
    return min(times), out


def plain_copy_ms(n_bytes, repeats):
    """A device buffer of n_bytes copied to pageable host memory with hipMemcpy."""
    hip = C.CDLL("libamdhip64.so")
    dev = C.c_void_p()
    assert hip.hipMalloc(C.byref(dev), C.c_size_t(n_bytes)) == 0
    try:
        assert hip.hipMemset(dev, 1, C.c_size_t(n_bytes)) == 0 and hip.hipDeviceSynchronize() == 0
        host = np.empty(n_bytes, np.uint8)
        host[:] = 0  # (touched: the pages exist, as a blob's do on its second save)

        def copy():
            assert hip.hipMemcpy(C.c_void_p(host.ctypes.data), dev, C.c_size_t(n_bytes), 2) == 0  # hipMemcpyDeviceToHost
        return best(copy, repeats)[0]
    finally:
        hip.hipFree(dev)


def measure(frame, fresh, repeats):
    lib = binding.load()
    info = frame.info()
    blob = frame.checkpoint()
    got = binding.checkpoint_inspect(blob)
    park = 528 * info["streams_parked"]
    out = {"streams": {k: got[k] for k in ("streams_finished", "streams_with_record", "streams_with_candidates", "streams_untouched")},
           "blob_bytes": int(got["total_bytes"]), "bytes_records": int(got["bytes_records"]), "bytes_pixels": int(got["bytes_pixels"]), "bytes_map": int(got["bytes_map"]),
           "park_record_bytes": park, "records_over_park": got["bytes_records"] / float(max(park, 1)), "blob_over_park": got["total_bytes"] / float(max(park, 1))}
    out["checkpoint_ms"] = best(frame.checkpoint, repeats)[0]
    buf, written = np.zeros(len(blob), np.uint8), C.c_size_t()

    def save():
        binding._check(lib.pt_frame_checkpoint_save(frame._h, binding._ptr(frame.image), binding._ptr(buf), C.c_size_t(len(buf)), C.byref(written)))
    out["save_ms"] = best(save, repeats)[0]
    assert buf.tobytes() == blob.tobytes()
    size = C.c_size_t()
    out["size_ms"] = best(lambda: binding._check(lib.pt_frame_checkpoint_size(frame._h, C.byref(size))), repeats)[0]

    def load():
        binding.Frame.restore(fresh, blob).close()
    out["load_ms"] = best(load, repeats)[0]
    out["inspect_ms"] = best(lambda: binding.checkpoint_inspect(blob), repeats)[0]
    out["plain_copy_of_park_records_ms"] = plain_copy_ms(max(park, 1), repeats)
    out["plain_copy_of_blob_bytes_ms"] = plain_copy_ms(len(blob), repeats)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="dragon")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--mesh-n", type=int, default=bench.parse_args([]).mesh_n)
    ap.add_argument("--quantum", type=int, default=8)
    ap.add_argument("--adaptive-passes", type=int, default=6)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--out", default=os.path.join("profiles", "checkpoint_probe.json"))
    args = ap.parse_args()
    sc, cam, label, _ = bench.build_workload(args.workload, args.width, args.height, args.mesh_n)
    gpu, fresh = binding.Scene(sc, device=0), binding.Scene(sc, device=0)
    out = {"workload": label, "frame": "%dx%d" % (args.width, args.height), "quantum": args.quantum, "repeats": args.repeats}
    try:
        for name, spp, passes in (("fixed", (64, 64), 1), ("adaptive", (16, 64), args.adaptive_passes)):
            frame = binding.Frame(gpu, cam, scenes.options(args.width, args.height, *spp), base_seed=args.seed)
            try:
                frame.set_progressive(args.quantum, passes)
                _, _, info = frame.render()
                if info["status"] == binding.PT_OK:
                    raise SystemExit("%s: the frame finished in %d passes; nothing to checkpoint" % (name, passes))
                out[name] = dict(measure(frame, fresh, args.repeats), spp=list(spp), passes=frame.progress()["passes_completed"])
                print("%-8s %s" % (name, json.dumps(out[name])), flush=True)
            finally:
                frame.close()
    finally:
        gpu.close()
        fresh.close()
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
