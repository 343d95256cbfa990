"""Where the time of bulk generation goes: sample / inner decode / decode / pack / copy, from two
`rocprofv3 --kernel-trace --stats -f csv` runs of profiles/generate_throughput.py --mode new --uint8 --reps 1:

    python profiles/generate_breakdown.py <dir of the --method ours run> <dir of the --method standard_gaussian run> <chunks per run>

The inner decoder and the decoder share kernels (dense layers), so names cannot tell them apart.  The standard_gaussian run has no inner
decoder and is otherwise the same loop, so the difference in launches per chunk IS the inner decoder's launch count; in the trace of the
"ours" run, ordered by start time, that many launches after each sampler launch are the inner decoder's and the rest, up to the packing
kernel, the decoder's.  Prints one JSON object: kernel milliseconds per group (both passes of the run: warm-up + one timed), device-to-host
copy milliseconds (the copies into pinned host memory are blit kernels on the copy stream: every launch off the compute stream), and the
launch counts the split rests on.  Result: profiles/generate_throughput.json, key "breakdown"."""
import csv
import glob
import json
import os
import sys


def rows(d, suffix):
    f = sorted(glob.glob(os.path.join(d, "**", "*" + suffix), recursive=True))
    assert f, "no *%s under %s" % (suffix, d)
    return list(csv.DictReader(open(f[0])))


def kernels(d):
    """-> (launches of the compute stream from the first draw on, launches of every other stream in that window: the copy stream's)."""
    k = [(int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"]), r["Kernel_Name"], r["Stream_Id"]) for r in rows(d, "kernel_trace.csv")]
    k.sort()
    first = next(i for i, r in enumerate(k) if is_sample(r[2]))
    k = k[first:]                                                    # (before the first draw: parameter initialisation, sampler prepare)
    main = k[0][3]
    return [r[:3] for r in k if r[3] == main], [r[:3] for r in k if r[3] != main]


def is_sample(n):
    return "sample_thread_kernel" in n or "sample_wave_kernel" in n


def main():
    (ours, copies), (sg, _), chunks = kernels(sys.argv[1]), kernels(sys.argv[2]), int(sys.argv[3])
    n_chunks = sum(is_sample(n) for _, _, n in ours)
    assert n_chunks == sum(is_sample(n) for _, _, n in sg) and n_chunks % chunks == 0, (n_chunks, chunks)
    assert (len(ours) - len(sg)) % n_chunks == 0, (len(ours), len(sg), n_chunks)
    n_inner = (len(ours) - len(sg)) // n_chunks
    ns = dict(sample=0, inner_decode=0, decode=0, pack=0)
    since = None
    for _, dur, name in ours:
        if is_sample(name):
            ns["sample"] += dur
            since = 0
        elif "images_to_u8" in name:
            ns["pack"] += dur
        else:
            since += 1
            ns["inner_decode" if since <= n_inner else "decode"] += dur
    sg_decode = sum(dur for _, dur, name in sg if not is_sample(name) and "images_to_u8" not in name)
    # the copies into pinned host memory are blit kernels on the copy stream (the memory-copy trace lists host-to-device transfers only)
    assert len(copies) == n_chunks and all("copyBuffer" in n for _, _, n in copies), (len(copies), n_chunks)
    ns["copy_to_host"] = sum(dur for _, dur, _ in copies)
    hidden = sum(1 for s0, dur, _ in copies if s0 + dur <= ours[-1][0])          # ended before the compute stream's last launch began
    span = (ours[-1][0] + ours[-1][1] - ours[0][0])
    print(json.dumps(dict(passes=n_chunks // chunks, chunks_per_pass=chunks, launches_per_chunk=len(ours) // n_chunks, inner_decode_launches_per_chunk=n_inner,
                          kernel_ms={k: round(v / 1e6, 3) for k, v in ns.items()}, compute_stream_kernel_ms=round((sum(ns.values()) - ns["copy_to_host"]) / 1e6, 3),
                          decode_ms_in_standard_gaussian_run=round(sg_decode / 1e6, 3),
                          copies=len(copies), copies_finished_under_later_compute=hidden, first_to_last_kernel_ms=round(span / 1e6, 3))))


if __name__ == "__main__":
    main()
