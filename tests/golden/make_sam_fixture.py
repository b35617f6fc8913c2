"""Writes tests/golden/spec_fixture.sam: the SAM text of the records of the committed spec_fixture.bam, from spec_fixture.json
alone (json only -- nothing of midas_amd, nothing of the BAM's bytes), in REVERSED order: the aligner writes reads as they come,
and the SAM decode (midas_sam_load_device) has to sort them.  Tags: NM:i when the record has one ("overflow" in the json is the
BAM's NM:I 4000000000, carried as INT32_MAX by both decoders), then YT:Z:UU.  A QUAL of 0xFF bytes is '*', an empty SEQ '*'.

  python tests/golden/make_sam_fixture.py        (rewrites the file; it is committed)
"""
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))
CIGAR_OPS = "MIDNSHP=X"


def main():
    with open(os.path.join(HERE, "spec_fixture.json")) as f:
        exp = json.load(f)
    lines = ["@HD\tVN:1.6\tSO:unsorted"] + ["@SQ\tSN:%s\tLN:%d" % (n, l) for n, l in exp["refs"]] + ["@PG\tID:make_sam_fixture"]
    recs = exp["records"]
    for k in reversed(range(len(recs))):
        r = recs[k]
        cigar = "".join("%d%s" % (w >> 4, CIGAR_OPS[w & 15]) for w in r["cigar"]) or "*"
        seq = r["seq"] or "*"
        qual = "*" if not r["qual"] or all(q == 0xFF for q in r["qual"]) else "".join(chr(q + 33) for q in r["qual"])
        nm = 4000000000 if r["nm"] == "overflow" else r["nm"]
        tags = (["NM:i:%d" % nm] if nm >= 0 else []) + ["YT:Z:UU"]
        lines.append("\t".join(["read%d" % k, str(r["flag"]), exp["refs"][r["refid"]][0], str(r["pos"] + 1), str(r["mapq"]), cigar,
                                "*", "0", "0", seq, qual] + tags))
    with open(os.path.join(HERE, "spec_fixture.sam"), "w", newline="\n") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote spec_fixture.sam (%d records)" % len(recs))


if __name__ == "__main__":
    main()
