#!/usr/bin/env python3
"""Refresh profiles/pmc_traffic.json["c3"] from one FETCH_SIZE pass, one
WRITE_SIZE pass and one SQ pass (GRBM_GUI_ACTIVE, SQ_LDS_IDX_ACTIVE,
SQ_INSTS_VALU) of `bench.py --steps 1 --warmup 1` at configs[2] (64 GiB):
the warm-up step is the store-mode call of the digest table (the hashing
hb_encode_first_kernel), the timed step the steady state that bench.py
measures (hb_encode_first_load_kernel), and the record describes the latter.
(Passes from before the digest table hold the hashing kernel only; they are
summarized as before, with no table term.)

HBM bytes per launch, corrected as MI355X_MICROARCH.md prescribes for gfx950:
FETCH_SIZE tallies the 128-B requests of wide coalesced reads at 64 B (the
streaming hb_read_kernel over the same 64 GiB reports exactly 1/2), so the
first pass's file reads count x2; what the HASHING first pass's FETCH_SIZE
holds beyond file / 2 is the per-block 1-byte prefix-image lookup (64-B
requests, counted 1:1); what the LOADING first pass fetches beyond the hashing
one is the digest table (32 B per block, two 16-B loads per lane, 2 KiB
contiguous per wave), counted x2 like the file reads when the counter shows
less than 3/4 of the table's size and 1:1 otherwise; WRITE_SIZE x 1024 B.
Usage: pmc_traffic.py FETCH.csv WRITE.csv SQ.csv"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from pmc_summary import summarize   # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILE = 64 << 30
BLOCKS = FILE // 512 + 1
TABLE = 32 * BLOCKS
HASHING, LOADING = "encode_first_kernel", "encode_first_load_kernel"


def pick(summ, part):
    for k, v in summ.items():
        if part in k:
            return v
    return {}


def compute(fetch_csv, write_csv, sq_csv):
    """The pmc_traffic.json["c3"] record of these three PMC passes."""
    f, w, q = summarize([fetch_csv]), summarize([write_csv]), summarize([sq_csv])
    kb = 1024
    table_mode = bool(pick(f, LOADING))
    first = LOADING if table_mode else HASHING
    ff, fr, fp = (pick(f, n).get("FETCH_SIZE", 0.0) for n in (first, "encode_retry", "prefix_kernel"))
    wf, wr, wp = (pick(w, n).get("WRITE_SIZE", 0.0) for n in (first, "encode_retry", "prefix_kernel"))
    fh = pick(f, HASHING).get("FETCH_SIZE", 0.0)     # the warm-up's store-mode call (or the only first pass)
    wh = pick(w, HASHING).get("WRITE_SIZE", 0.0)
    p3 = fh * kb - FILE / 2
    counted = (ff - fh) * kb if table_mode else 0.0
    factor = 2 if table_mode and counted < 0.75 * TABLE else 1
    table = counted * factor
    fetch = FILE + p3 + table + (fr + fp) * kb
    write = (wf + wr + wp) * kb
    sq = pick(q, first)
    sqh = pick(q, HASHING)
    per_iter = lambda s: round(s.get("SQ_INSTS_VALU", 0.0) / (BLOCKS / 64.0), 1)   # noqa: E731
    rec = {
        "file_bytes": FILE,
        "hbm_bytes_per_launch": int(round(fetch + write)),
        "fetch_bytes_corrected": int(round(fetch)),
        "write_bytes": int(round(write)),
        "breakdown": {"sector_reads": FILE, "prefix_image_lookups": int(round(p3)),
                      "digest_table_loads": int(round(table)),
                      "retry_list_reads": int(round(fr * kb)), "tag_and_retry_list_writes": int(round((wf + wr) * kb)),
                      "prefix_image_build": int(round((fp + wp) * kb))},
        "raw_kB": {"FETCH_SIZE_first": ff, "FETCH_SIZE_retry": fr, "FETCH_SIZE_prefix": fp,
                   "WRITE_SIZE_first": wf, "WRITE_SIZE_retry": wr, "WRITE_SIZE_prefix": wp,
                   "FETCH_SIZE_first_hashing": fh, "WRITE_SIZE_first_hashing": wh},
        "digest_table": {"mode": "load" if table_mode else "none", "bytes": TABLE if table_mode else 0,
                         "fetch_counted": int(round(counted)), "fetch_factor": factor,
                         "store_call_extra_writes": int(round((wh - wf) * kb)) if table_mode else 0},
        "correction": __doc__.split("HBM bytes per launch, ")[1].split("Usage")[0].strip().replace("\n", " "),
        "source": "%s, %s (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE, one per pass, bench.py --steps 1 --warmup 1)"
                  % (fetch_csv, write_csv),
        "ratio_to_algorithmic": round((fetch + write) / (FILE + FILE // 512 * 32), 3),
        "lds_busy": round(sq.get("lds_busy", 0.0), 3),
        "held_clock_ghz": round(sq.get("clock_ghz", 0.0), 3),
        "valu_wave_instr_per_cu_clk": round(sq.get("valu_per_cu_clk", 0.0), 3),
        "valu_wave_instr_per_wave_iteration": per_iter(sq),
        "first_pass_ms_under_pmc": round(sq.get("duration_ms", 0.0), 3),
        "hashing_first_pass": {"lds_busy": round(sqh.get("lds_busy", 0.0), 3),
                               "held_clock_ghz": round(sqh.get("clock_ghz", 0.0), 3),
                               "valu_wave_instr_per_cu_clk": round(sqh.get("valu_per_cu_clk", 0.0), 3),
                               "valu_wave_instr_per_wave_iteration": per_iter(sqh),
                               "ms_under_pmc": round(sqh.get("duration_ms", 0.0), 3)},
        "source_pmc": "%s (first-pass kernel %s, one rocprofv3 --pmc pass): held clock = GRBM_GUI_ACTIVE / 8 XCDs / "
                      "duration; lds_busy = SQ_LDS_IDX_ACTIVE / (256 CUs x GRBM_GUI_ACTIVE/8); valu = SQ_INSTS_VALU / "
                      "(256 CUs x GRBM_GUI_ACTIVE/8); SQ_LDS_BANK_CONFLICT = %d"
                      % (sq_csv, "hb_" + first, sq.get("SQ_LDS_BANK_CONFLICT", -1)),
    }
    return rec


def main(fetch_csv, write_csv, sq_csv):
    rec = compute(fetch_csv, write_csv, sq_csv)
    path = os.path.join(ROOT, "profiles", "pmc_traffic.json")
    d = json.load(open(path))
    d["c3"] = rec
    json.dump(d, open(path, "w"), indent=1)
    print(json.dumps(rec, indent=1))


if __name__ == "__main__":
    main(*sys.argv[1:4])
