"""The int16 streaming entries (vad_stream_hops_i16, vad_stream_hop_i16,
vad_stream_push_hop_i16) refuse bad arguments with a negative VAD_E* code
before any HIP call, exactly as their f32 twins do: runs on the CPU, the
calls in a child process so that a crash fails this test and not the run.
Handles and pointers that a refusal must not touch are passed as the
non-null dummy address 1."""
import json
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r'''
import json, sys
sys.path.insert(0, sys.argv[1])
from vad_amd import _lib
L = _lib.lib()
N, P = None, 1  # NULL, a non-null address no refusal may dereference
res = {}
def call(tag, name, *args):
    res[tag + ": " + name + repr(args)] = [int(getattr(L, name)(*args)), int(getattr(L, name.replace("_i16", ""))(*args))]
S = 10
# vad_stream_push_hop_i16(frames, frame_stride, frame_len, hop, hop_stride, hop_len, n_streams, stream)
def push(tag, frames=P, fs=400, fl=400, hop=P, hs=160, hl=160, n=S):
    call(tag, "vad_stream_push_hop_i16", frames, fs, fl, hop, hs, hl, n, N)
push("null frames", frames=N)
push("null hop", hop=N)
push("null both", frames=N, hop=N)
push("frame_len 1025", fs=1025, fl=1025)
push("frame_len 0", fl=0)
push("hop_len > frame_len", hs=500, hl=401)
push("hop_len 0", hl=0)
push("frame stride short", fs=399)
push("hop stride short", hs=159)
push("negative streams", n=-1)
# vad_stream_hop_i16(plan, ffn, frames, frame_stride, frame_len, hop, hop_stride, hop_len, n_streams,
#                    ring, count, labels, stream)
def hop1(tag, plan=P, ffn=P, frames=P, fs=400, fl=400, hop=P, hs=160, hl=160, n=S, ring=P, count=P, labels=P):
    call(tag, "vad_stream_hop_i16", plan, ffn, frames, fs, fl, hop, hs, hl, n, ring, count, labels, N)
hop1("null plan", plan=N)
hop1("null ffn", ffn=N)
hop1("null all", plan=N, ffn=N, frames=N, hop=N, ring=N, count=N, labels=N)
for k in ("frames", "hop", "ring", "count", "labels"):
    hop1("null " + k, **{k: N})
hop1("frame_len 1025", fs=1025, fl=1025)
hop1("hop_len > frame_len", hs=500, hl=401)
hop1("frame stride short", fs=399)
hop1("hop stride short", hs=159)
hop1("negative streams", n=-1)
# vad_stream_hops_i16(plan, ffn, frames, frame_stride, frame_len, hop, hop_stride, hop_len, n_streams,
#                     n_hops, hop_block_stride, ring, count, labels, label_block_stride, stream)
def hops(tag, plan=P, ffn=P, frames=P, fs=400, fl=400, hop=P, hs=160, hl=160, n=S, k=8, bs=1600, ring=P, count=P,
         labels=P, ls=S):
    call(tag, "vad_stream_hops_i16", plan, ffn, frames, fs, fl, hop, hs, hl, n, k, bs, ring, count, labels, ls, N)
hops("null plan", plan=N)
hops("null ffn", ffn=N)
hops("null all", plan=N, ffn=N, frames=N, hop=N, ring=N, count=N, labels=N)
for k in ("frames", "hop", "ring", "count", "labels"):
    hops("null " + k, **{k: N})
hops("frame_len 1025", fs=1025, fl=1025)
hops("hop_len > frame_len", hs=500, hl=401)
hops("frame stride short", fs=399)
hops("hop stride short", hs=159)
hops("negative streams", n=-1)
hops("negative hops", k=-1)
hops("zero block stride", bs=0)
hops("negative block stride", bs=-1600)
hops("overlapping block stride", bs=9 * 160 + 159)
hops("overlapping stream-major", hs=8 * 160 - 1, bs=160)
hops("label stride below n_streams", ls=S - 1)
hops("label stride zero", ls=0)
# nothing to do is VAD_OK, as for the f32 entries (and still before any HIP call)
ok = {
    "push 0 streams": int(L.vad_stream_push_hop_i16(N, 400, 400, N, 160, 160, 0, N)),
    "hop 0 streams": int(L.vad_stream_hop_i16(P, P, N, 400, 400, N, 160, 160, 0, N, N, N, N)),
    "hops 0 hops": int(L.vad_stream_hops_i16(P, P, N, 400, 400, N, 160, 160, S, 0, 0, N, N, N, 0, N)),
}
print(json.dumps({"calls": res, "ok": ok}))
'''


def test_int16_stream_entries_refuse_bad_arguments():
    r = subprocess.run([sys.executable, "-c", CHILD, REPO], capture_output=True, text=True, timeout=300, cwd=REPO)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    out = json.loads([x for x in r.stdout.splitlines() if x.startswith("{")][-1])
    assert len(out["calls"]) == 43  # every call() above has a distinct tag
    bad = {k: v for k, v in out["calls"].items() if v[0] >= 0}
    assert not bad, bad  # every refusal is a negative VAD_E* code
    differ = {k: v for k, v in out["calls"].items() if v[0] != v[1]}
    assert not differ, differ  # and the f32 twin's code: the same checks in the same order
    assert out["ok"] == {k: 0 for k in out["ok"]}, out["ok"]


def test_stream_batch_refuses_other_input_dtypes():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("StreamBatch needs a device to construct")
    from vad_amd.ffn import TOPOLOGY_REF39, FFNClassifier, random_layers
    from vad_amd.stream import StreamBatch
    clf = FFNClassifier(random_layers(TOPOLOGY_REF39, seed=1))
    for dt in (torch.float64, torch.float16, torch.int32, torch.uint8):
        with pytest.raises(ValueError, match="input_dtype"):
            StreamBatch(2, clf, input_dtype=dt)
    assert StreamBatch(2, clf, input_dtype=torch.int16).inputs.dtype == torch.int16
    assert StreamBatch(2, clf).inputs.dtype == torch.float32
