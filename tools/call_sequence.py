#!/usr/bin/env python3
"""The runtime calls of a run, one per line, from a `rocprofv3 --hip-trace --kernel-trace --output-format csv` directory:

    call_sequence.py DIR                 the whole run: "<HIP function> <kernels it dispatched>"
    call_sequence.py DIR --steps N       the last N steps only (a step starts at the call that dispatches k_frame_wave)
    call_sequence.py OLD NEW [--steps N] both, compared line for line; exit status 1 if they differ

A line is the API name plus, for a launch, the kernel's name (template arguments kept, parameter list dropped); a graph
launch carries every kernel of the graph, sorted by name (branches of a graph start in an order that varies from replay
to replay).  Calls that only ask (hipGetLastError, hipGetDevice, ...)
are left out.  The CSV that rocprofv3 (ROCm 7) writes holds no arguments (its columns: Domain, Function, Process_Id, Thread_Id, Correlation_Id,
Start_Timestamp, End_Timestamp; --header prints what the trace at hand has): streams and events cannot be compared from it."""
import csv, glob, os, re, sys

ASKS = {"hipGetLastError", "hipPeekAtLastError", "hipGetDevice", "hipSetDevice", "hipGetDeviceCount", "hipDeviceGetAttribute",
        "hipGetDevicePropertiesR0600", "hipStreamIsCapturing", "hipStreamGetCaptureInfo", "hipStreamGetCaptureInfo_v2",
        "hipEventQuery", "hipStreamQuery", "hipDriverGetVersion", "hipRuntimeGetVersion", "hipDeviceGetStreamPriorityRange",
        "__hipPushCallConfiguration", "__hipPopCallConfiguration", "hipGetErrorString", "hipPointerGetAttribute",
        "hipPointerGetAttributes", "hipCtxGetCurrent", "hipDevicePrimaryCtxGetState", "hipMemGetInfo", "hipFuncGetAttributes"}


def one(d, pattern):
    hits = sorted(glob.glob(os.path.join(d, "**", pattern), recursive=True))
    if not hits:
        sys.exit("no %s under %s" % (pattern, d))
    return hits[0]


def short(kernel):
    name = re.sub(r"\(.*", "", kernel.replace("void ", "", 1)) if not kernel.endswith(".kd") else kernel[:-3]
    return name.strip()


def sequence(d, header=False):
    api = list(csv.DictReader(open(one(d, "*hip_api_trace.csv"))))
    ker = list(csv.DictReader(open(one(d, "*kernel_trace.csv"))))
    if header:
        print("# hip_api_trace.csv columns: %s" % ", ".join(api[0].keys()))
    by_corr = {}
    for k in ker:
        by_corr.setdefault(k["Correlation_Id"], []).append(short(k["Kernel_Name"]))
    for names in by_corr.values():          # a graph's branches run side by side: the order its kernels START in is not the
        names.sort()                        # host's doing and differs from replay to replay -- listed by name
    lines = []
    for r in sorted(api, key=lambda r: int(r["Start_Timestamp"])):
        if r["Function"] in ASKS:
            continue
        lines.append((r["Function"] + " " + " ".join(by_corr.get(r["Correlation_Id"], []))).rstrip())
    return lines


def last_steps(lines, n):
    starts = [i for i, l in enumerate(lines) if "k_frame_wave" in l]
    if len(starts) <= n:
        sys.exit("fewer than %d steps in the trace" % (n + 1))
    return lines[starts[-n - 1]:starts[-1]]            # n whole steps, the run's very last (cut short by its end) left out


def main(argv):
    args = [a for a in argv if not a.startswith("--")]
    n = int(argv[argv.index("--steps") + 1]) if "--steps" in argv else 0
    if n:
        args.remove(str(n))
    seqs = [sequence(d, "--header" in argv) for d in args]
    if n:
        seqs = [last_steps(s, n) for s in seqs]
    if len(seqs) == 1:
        print("\n".join(seqs[0]))
        return 0
    a, b = seqs
    diff = [i for i in range(min(len(a), len(b))) if a[i] != b[i]]
    print("# %d calls in old, %d in new, %s" % (len(a), len(b), "identical line for line" if a == b else
                                                 "first difference at line %d" % (diff[0] + 1 if diff else min(len(a), len(b)) + 1)))
    if a != b and diff:
        print("# old: %s\n# new: %s" % (a[diff[0]], b[diff[0]]))
    return 0 if a == b else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
