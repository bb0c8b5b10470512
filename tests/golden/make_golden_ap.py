#!/usr/bin/env python3 -B
"""Golden vectors for the detector evaluation's AP tables by IMPORTING the reference.

Runs only in the build container (needs /root/reference).  The functions under test are the reference's own
`lib/datasets/voc_eval.py` -- voc_eval for the two classes, voc_eval_hand for the four constraints, both `use_07_metric` values
-- imported under the two aliases the installed numpy no longer has (np.bool = bool, np.int = int: names, no arithmetic).  They
are fed as the evaluation feeds them: the annotation cache as the pickle voc_eval would have written, and the two detection text
files, one line per selected record in image-index order, every number formatted as pascal_voc.py:339-343 formats it.

    python -B tests/golden/make_golden_ap.py      ->  tests/golden/det_ap.npz

The inputs are tests/ap_cases.py at shape (4, 8, 3) without the tie kinds, an image's padding hands carrying an object box when
its own hands do (the reference stacks them into one array), and with the selected records' scores replaced by values whose
three-decimal forms are all distinct: the reference leaves the order of equal scores to numpy's sort, so only then is its result
independent of it.  That condition is asserted here; ties are covered against the rule only.
"""
from __future__ import annotations

import pickle
import sys
import tempfile
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
REF = Path("/root/reference")
sys.dont_write_bytecode = True
sys.path.insert(0, str(HERE.parent))

SHAPE = (4, 8, 3)
CONSTRAINTS = ("handstate", "handside", "objectbbox", "all")
SCORE_MIN = np.float32(0.1)
KEEP = (np.float32(0.8125), np.float32(0.4375))           # the half-way kind's scores stay as they are


def selected(batch, n, label):
    count = int(batch["count"][n])
    return [k for k in range(count) if batch["scores"][n, k] > SCORE_MIN and batch["labels"][n, k] == label]


def rescore(batches):
    """distinct three-decimal scores for all selected records, each image's order kept"""
    step = 0
    for batch in batches:
        for n in range(batch["count"].shape[0]):
            for k in range(int(batch["count"][n])):
                s = batch["scores"][n, k]
                if not s > SCORE_MIN or batch["labels"][n, k] not in (1, 2) or s in KEEP:
                    continue
                batch["scores"][n, k] = np.float32(0.995 - 0.001 * step)
                step += 1
    assert 0.995 - 0.001 * step > 0.82, "the new scores must stay above the half-way kind's"


def rows_of_class(batch, n, label):
    """trainval_net_fcos.py:132-158 for one image and class: float32 rows (box, score, contact, dxdymags, side, 1)"""
    ks = selected(batch, n, label)
    rows = np.zeros((len(ks), 11), np.float32)
    for r, k in enumerate(ks):
        rows[r, 0:4], rows[r, 4], rows[r, 5] = batch["boxes"][n, k], batch["scores"][n, k], batch["contacts"][n, k]
        rows[r, 6:9], rows[r, 9], rows[r, 10] = batch["dxdymags"][n, k], batch["sides"][n, k], 1.0
    return rows


def line_of(name, row):
    """one record as the results file holds it: three decimals for the score, the vector and the side, one decimal for the
    float32 coordinate + 1, the contact state as an int"""
    fields = [name, format(row[4], ".3f")] + [format(row[c] + 1, ".1f") for c in range(4)] + [str(int(row[5]))]
    fields += [format(row[c], ".3f") for c in (6, 7, 8, 9, 10)]
    return " ".join(fields) + "\n"


def main():
    np.bool, np.int = bool, int                               # the names voc_eval.py still uses
    sys.path.insert(0, str(REF / "lib" / "datasets"))
    import voc_eval as ve                                     # the reference's own file
    import ap_cases

    kinds = [k for k in ap_cases.KINDS if k.__name__ not in ap_cases.TIE_KINDS]
    case = ap_cases.cases(SHAPE, kinds=kinds, uniform=True)
    batches = [{k: v.copy() for k, v in b.items()} for b in case["batches"]]
    rescore(batches)
    batch = ap_cases.concat(batches)
    names, recs = case["image_index"], case["recs"]
    assert len(names) >= 12 and set(k.__name__ for k in kinds) <= set(case["kinds"])

    per_image = {}
    for n, image in enumerate(batch["image_ids"].tolist()):
        objs, hands = rows_of_class(batch, n, 1), rows_of_class(batch, n, 2)
        if hands.shape[0] == 0:                               # trainval_net_fcos.py:161-169: no hands, no objects either
            objs = objs[:0]
        per_image[image] = (objs, hands)
    lines = {"targetobject": [], "hand": []}
    for image, name in enumerate(names):
        if image in per_image:
            for cls, rows in zip(("targetobject", "hand"), per_image[image]):
                lines[cls] += [line_of(name, row) for row in rows]
    for cls, ls in lines.items():
        shown = [l.split(" ")[1] for l in ls]
        assert len(set(shown)) == len(shown), f"equal rounded scores among the {cls} records"
    assert "0.812" in [l.split(" ")[1] for l in lines["hand"]]

    out = {k: v for k, v in batch.items()}
    out["image_index"] = np.array(names)
    out["kinds"] = np.array(case["kinds"])
    with tempfile.TemporaryDirectory() as tmp:
        tmp = Path(tmp)
        imageset = tmp / "test.txt"
        imageset.write_text("".join(n + "\n" for n in names))
        with open(str(imageset) + "_annots.pkl", "wb") as f:   # where voc_eval looks for its cache
            pickle.dump(recs, f)
        for cls, ls in lines.items():
            (tmp / f"det_{cls}.txt").write_text("".join(ls))
        detpath, annopath = str(tmp / "det_{:s}.txt"), str(tmp / "unused_{:s}.xml")
        for m07 in (False, True):
            tag = "07" if m07 else "10"
            res = {"targetobject": ve.voc_eval(detpath, annopath, str(imageset), "targetobject", str(tmp), ovthresh=0.5, use_07_metric=m07),
                   "hand": ve.voc_eval(detpath, annopath, str(imageset), "hand", str(tmp), ovthresh=0.5, use_07_metric=m07)}
            for c in CONSTRAINTS:
                res["hand+" + c] = ve.voc_eval_hand(detpath, annopath, str(imageset), "hand", str(tmp), ovthresh=0.5,
                                                    use_07_metric=m07, constraint=c)
            for name, (rec, prec, ap) in res.items():
                out[f"rec_{tag}_{name}"], out[f"prec_{tag}_{name}"], out[f"ap_{tag}_{name}"] = rec, prec, np.float64(ap)
    # the annotation cache, record by record (the test rebuilds the dict from these)
    flat = [(name, r) for name in names for r in recs[name]]
    out["rec_image"] = np.array([n for n, _ in flat])
    out["rec_name"] = np.array([r["name"] for _, r in flat])
    out["rec_bbox"] = np.array([r["bbox"] for _, r in flat], np.int32).reshape(-1, 4)
    out["rec_fields"] = np.array([[r["difficult"], r["handstate"], r["leftright"], int(r["objectbbox"] is not None)] for _, r in flat],
                                 np.int32).reshape(-1, 4)
    out["rec_objectbbox"] = np.array([r["objectbbox"] or [0.0] * 4 for _, r in flat], np.float64).reshape(-1, 4)
    np.savez_compressed(HERE / "det_ap.npz", **out)
    print("wrote", HERE / "det_ap.npz", len(names), "images,", {c: len(l) for c, l in lines.items()}, "records; AP",
          {k[6:]: float(v) for k, v in out.items() if k.startswith("ap_10_")})


if __name__ == "__main__":
    main()
