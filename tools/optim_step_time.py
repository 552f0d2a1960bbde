"""Times one optimizer step -- global gradient-norm clip + update -- over the parameters of bench.py's model (full-size
DeepSpeech2: 48 float32 tensors, about 118 M elements; random gradients), once for Adam and once for SGD with momentum.

  torch_foreach      ``torch.nn.utils.clip_grad_norm_(foreach=True)`` + ``torch.optim.*(foreach=True)``
  torch_fused        the same clip + ``torch.optim.*(fused=True)``, where this torch build accepts it
  project            ``myrtlespeech_amd.optim.*`` with ``max_grad_norm``: one pass for the norm, one for the update

``max_norm`` is 1e9, so no arm's clip bites and every repeat does the same work (torch's clip multiplies the gradients by the
clamped coefficient whether it bites or not).  Every arm owns a copy of the parameters and of the gradients.  The arms of a
group alternate in one process after one untimed call each; a call is timed with the host clock around work that ends in a
device synchronise; the median of ``--repeats`` (7) is the figure, min and max beside it.

Per arm it records the bytes the arm's passes must move at the least (per element: 4 for the norm, 8 for a clip that
rewrites the gradients, 28 for an Adam update -- read p, g, m, v, write p, m, v -- and 20 for SGD with momentum) and the fraction
of the HBM rate (bench.py's HBM_PEAK_GBS) that the time implies.  The floor is the project arm's: 32 bytes per element for
Adam, 24 for SGD with momentum.

Last, one whole ``fit()`` training step of the same model (forward with ``differentiable=True``, CTC loss, backward, fused
clip + Adam, ``zero_grad``), and the same with the step suppressed, at bench.py's batch.  No thresholds: the numbers are the
output.  There is no CPU path.

    python tools/optim_step_time.py [--repeats 7] [--out profiles/optim_step_time.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import torch  # noqa: E402

import bench  # noqa: E402

MAX_NORM = 1e9
KINDS = {"adam": dict(torch="Adam", kw=dict(lr=1e-3), update_bytes=28),
         "sgd_momentum": dict(torch="SGD", kw=dict(lr=1e-3, momentum=0.9), update_bytes=20)}


def spread(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4), "repeats": len(v)}


def timed(arms, repeats):
    for fn in arms.values():                                              # untimed
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in arms}
    for _ in range(repeats):
        for k, fn in arms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t0) * 1e3)
    return ms


def progress(what):
    print(f"optim_step_time: {what}", file=sys.stderr, flush=True)


def copies(shapes, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    params = [torch.nn.Parameter(torch.randn(s, generator=g, device="cuda") * 0.05) for s in shapes]
    for p in params:
        p.grad = torch.randn(p.shape, generator=g, device="cuda") * 0.01
    return params


def optimizer_arms(kind, shapes):
    """(arms, bytes per element each arm must move, notes)."""
    from myrtlespeech_amd import optim
    spec = KINDS[kind]
    arms, per_element, notes = {}, {}, {}

    def torch_arm(name, **switch):
        params = copies(shapes, 1)
        try:
            opt = getattr(torch.optim, spec["torch"])(params, **spec["kw"], **switch)

            def step():
                torch.nn.utils.clip_grad_norm_(params, MAX_NORM, foreach=True)
                opt.step()
            step()
            torch.cuda.synchronize()
        except (RuntimeError, TypeError, ValueError) as e:
            notes[name] = f"not accepted by this torch build: {e}"
            return
        arms[name] = step
        per_element[name] = 4 + 8 + spec["update_bytes"]

    torch_arm("torch_foreach", foreach=True)
    torch_arm("torch_fused", fused=True)
    params = copies(shapes, 1)
    own = getattr(optim, spec["torch"])(params, max_grad_norm=MAX_NORM, **spec["kw"])
    arms["project"] = own.step
    per_element["project"] = 4 + spec["update_bytes"]
    return arms, per_element, notes


def fit_arms():
    from myrtlespeech_amd import optim
    from myrtlespeech_amd.loss.ctc_loss import CTCLoss
    from myrtlespeech_amd.model.seq_to_seq import SeqToSeq
    from myrtlespeech_amd.run.callbacks import Callback
    from myrtlespeech_amd.run.train import fit
    model = bench.build_model()
    model.rnn.check_status = False
    s = SeqToSeq(model, CTCLoss(), [])
    s.optim = optim.Adam(s.model.parameters(), lr=1e-4, max_grad_norm=5.0)
    n = bench.BATCH_PER_GPU
    x = torch.randn(n, 1, bench.FEATURES, bench.FRAMES).cuda()
    lens = torch.full((n,), bench.FRAMES, dtype=torch.int64)
    y, y_lens = torch.randint(0, bench.VOCAB - 1, (n, 120)), torch.full((n,), 120, dtype=torch.int64)
    loader = [((x, lens), (y, y_lens))]

    class SkipStep(Callback):
        def on_backward_end(self, **kw):
            return {"skip_step": True}

    return {"fit_step": lambda: fit(s, 1, loader), "fit_step_without_optimizer_step": lambda: fit(s, 1, loader, callbacks=[SkipStep()])}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--no-fit", action="store_true", help="skip the whole training step")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optim_step_time.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("optim_step_time: a HIP device is required; there is no CPU path")
    shapes = [tuple(p.shape) for p in bench.build_model().parameters()]
    elements = sum(int(torch.Size(s).numel()) for s in shapes)
    out = {"tool": "tools/optim_step_time.py", "commit": a.commit, "torch": torch.__version__,
           "parameters": {"tensors": len(shapes), "elements": elements, "model": "bench.py build_model()"},
           "max_norm": MAX_NORM, "hbm_peak_gbs": bench.HBM_PEAK_GBS,
           "statistic": "host clock around calls ending in a device synchronise, per call, ms; the arms of a group alternate in "
                        "one process after one untimed call each; median of the repeats"}
    for kind, spec in KINDS.items():
        progress(kind)
        arms, per_element, notes = optimizer_arms(kind, shapes)
        ms = timed(arms, a.repeats)
        rec = {"floor_bytes_per_element": 4 + spec["update_bytes"], "arms": {}, "not_run": notes}
        for k, v in ms.items():
            med = statistics.median(v)
            nbytes = per_element[k] * elements
            rec["arms"][k] = {"ms": spread(v), "bytes_per_element": per_element[k], "bytes": nbytes,
                              "fraction_of_hbm_rate": round(nbytes / (med * 1e-3) / (bench.HBM_PEAK_GBS * 1e9), 4)}
        for k in ms:
            if k != "project":
                rec[f"project_over_{k}"] = round(statistics.median(ms["project"]) / statistics.median(ms[k]), 3)
        out[kind] = rec
        del arms
        torch.cuda.empty_cache()
    if not a.no_fit:
        progress("one whole fit() training step")
        ms = timed(fit_arms(), a.repeats)
        out["fit"] = {f"{k}_ms": spread(v) for k, v in ms.items()}
        out["fit"]["batch"] = [bench.BATCH_PER_GPU, 1, bench.FEATURES, bench.FRAMES]
        out["fit"]["optimizer_share_ms"] = round(statistics.median(ms["fit_step"])
                                                 - statistics.median(ms["fit_step_without_optimizer_step"]), 4)
    text = json.dumps(out, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
