"""What the recorder tests share (tests/test_recorder.py on the GPU, tests/test_recorder_cpu.py on the CPU): the episode
splitter over rows of aleppo_rec_step - the rule the trainer's writer follows (trainer/recorder.hpp) - and parsers of the two
files the writer produces, uncompressed YUV4MPEG2 (`Cmono`) and the tab-separated step table."""
import re

import numpy as np

TSV_COLUMNS = ("ordinal", "action", "reward", "value", "start", "terminated", "truncated", "game_over", "lives")


def split_episodes(steps):
    """rows of REC_STEP_DTYPE (or anything with ordinal / start / terminated / truncated columns) -> (episodes, open):
    episodes = [(first_row, last_row, whole)] in order, one per row with start = 1 that is followed by a row with
    terminated or truncated; whole is False where the ordinals between the two are not consecutive (such an episode is
    skipped by the writer, but still counted).  Rows in front of the first start row belong to no episode.  open = the first
    row of the unfinished episode at the end, or None."""
    episodes, first, whole = [], None, True
    for r in range(len(steps)):
        if steps["start"][r]:
            first, whole = r, True
        elif first is not None and int(steps["ordinal"][r]) != int(steps["ordinal"][r - 1]) + 1:
            whole = False
        if first is not None and (steps["terminated"][r] or steps["truncated"][r]):
            episodes.append((first, r, whole))
            first = None
    return episodes, first


def parse_y4m(path):
    """-> (header dict with W, H, F (the rate as written, e.g. "15:1"), I, A, C; frames uint8 [n, H, W])"""
    blob = open(path, "rb").read()
    nl = blob.index(b"\n")
    words = blob[:nl].decode("ascii").split(" ")
    assert words[0] == "YUV4MPEG2", words
    hdr = {w[0]: w[1:] for w in words[1:]}
    w, h = int(hdr["W"]), int(hdr["H"])
    assert hdr["C"] == "mono", hdr
    rec = len(b"FRAME\n") + w * h
    body = blob[nl + 1:]
    assert len(body) % rec == 0, (len(body), rec)
    frames = np.frombuffer(body, np.uint8).reshape(-1, rec)
    assert all(bytes(f[:6]) == b"FRAME\n" for f in frames)
    return hdr, frames[:, 6:].reshape(-1, h, w).copy()


def parse_tsv(path):
    """-> (structured rows with TSV_COLUMNS, logits float32 [n, A]); floats were written as %.9g, which round-trips float32"""
    rows, logits = [], []
    for line in open(path).read().splitlines():
        f = line.split("\t")
        assert len(f) > len(TSV_COLUMNS) and all(re.fullmatch(r"[-+0-9.eEinfa]+", x) for x in f), line
        rows.append((int(f[0]), int(f[1]), np.float32(f[2]), np.float32(f[3])) + tuple(int(x) for x in f[4:9]))
        logits.append([np.float32(x) for x in f[9:]])
    dt = np.dtype([("ordinal", "<u8"), ("action", "<i4"), ("reward", "<f4"), ("value", "<f4"), ("start", "u1"),
                   ("terminated", "u1"), ("truncated", "u1"), ("game_over", "u1"), ("lives", "<i4")])
    return np.array(rows, dt), np.array(logits, np.float32).reshape(len(rows), -1)
