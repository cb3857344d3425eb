"""Output writers — byte-format-compatible with the reference.

  *_biomarkers.txt  G2Vec.py:127-131
  *_lgroups.txt     G2Vec.py:159-165
  *_vectors.txt     G2Vec.py:203-215 (values printed \t%.6f)
  *_scores.txt      opt-in per-gene scores table (not in the reference)
  *_neighbors.txt   opt-in nearest-gene table (not in the reference)
"""
from __future__ import annotations

from typing import Iterable, Optional, Sequence

import numpy as np


def write_biomarkers(result_name: str, biomarkers: Iterable[str]) -> str:
    out = result_name + "_biomarkers.txt"
    with open(out, "w") as f:
        f.write("GeneSymbol\n")
        for g in biomarkers:
            f.write(f"{g}\n")
    return out


def write_lgroups(result_name: str, lgroup_idx: Sequence[int], genes: Sequence[str]) -> str:
    out = result_name + "_lgroups.txt"
    with open(out, "w") as f:
        f.write("GeneSymbol\tLgroup(0:good,1:poor,2:other)\n")
        for gene, grp in zip(genes, lgroup_idx):
            f.write("%s\t%d\n" % (gene, int(grp)))
    return out


def write_vectors(result_name: str, mat: np.ndarray, genes: Sequence[str],
                  engine: str = "auto") -> str:
    """engine: 'numpy' | 'pandas' | 'auto' (pandas above 5M values — its C
    csv writer is ~10x faster on the 1M-gene x 512 = 3.7 GB output)."""
    out = result_name + "_vectors.txt"
    h = mat.shape[1]
    if engine == "auto":
        engine = "pandas" if mat.size > 5_000_000 else "numpy"
    if engine == "pandas":
        import pandas as pd
        df = pd.DataFrame(mat, index=np.asarray(genes, dtype=str),
                          columns=[f"V{i}" for i in range(h)])
        df.index.name = "GeneSymbol"
        df.to_csv(out, sep="\t", float_format="%.6f", lineterminator="\n")
        return out
    header = "GeneSymbol" + "".join("\tV%d" % i for i in range(h)) + "\n"
    # vectorized "%.6f" formatting; byte format identical to the
    # reference's \t%.6f (G2Vec.py:214)
    cells = np.char.mod("%.6f", mat.astype(np.float64))
    rows = np.char.add(np.asarray(genes, dtype=str),
                       ["\t" + "\t".join(r) for r in cells])
    with open(out, "w") as f:
        f.write(header)
        f.write("\n".join(rows))
        f.write("\n")
    return out


def write_scores(result_name: str, genes: Sequence[str],
                 lgroup_idx: Sequence[int], scores: dict,
                 perm: Optional[dict] = None) -> str:
    """<name>_scores.txt: one tab-separated row per gene, in gene order.
    Columns GeneSymbol, Lgroup, d_score, t_score (raw values), gene_score
    (the within-L-group 0.5*(minmax d + minmax t) the selection ranks by; NA
    outside L-groups 0 and 1), biomarker (0/1) and, with perm (the dict of
    scoring.permutation_pvalues), p_perm, q_bh, p_maxT. Scores are printed
    %.6f, p-values %.6g. When scores carries "auc" (the rank-sum statistic
    was scored), the t_score column is named z_ranksum and auc follows it.
    When scores carries "silhouette" (f64 [G], or None where the split has
    fewer than two non-empty L-groups) with "nearest_lgroup", the columns
    silhouette (%.6f) and nearest_lgroup (%d) follow biomarker; NA for
    None."""
    out = result_name + "_scores.txt"
    ranksum = "auc" in scores
    cols = ["GeneSymbol", "Lgroup", "d_score"] + (
        ["z_ranksum", "auc"] if ranksum else ["t_score"]) + [
        "gene_score", "biomarker"]
    sil = "silhouette" in scores
    if sil:
        cols += ["silhouette", "nearest_lgroup"]
    if perm is not None:
        cols += ["p_perm", "q_bh", "p_maxT"]
    gs = np.asarray(scores["gene_score"], dtype=np.float64)
    with open(out, "w") as f:
        f.write("\t".join(cols) + "\n")
        for i, gene in enumerate(genes):
            row = [str(gene), "%d" % int(lgroup_idx[i]),
                   "%.6f" % float(scores["d_score"][i]),
                   "%.6f" % float(scores["t_score"][i])] + (
                   ["%.6f" % float(scores["auc"][i])] if ranksum else []) + [
                   "NA" if np.isnan(gs[i]) else "%.6f" % gs[i],
                   "%d" % int(scores["is_biomarker"][i])]
            if sil and scores["silhouette"] is None:
                row += ["NA", "NA"]
            elif sil:
                row += ["%.6f" % float(scores["silhouette"][i]),
                        "%d" % int(scores["nearest_lgroup"][i])]
            if perm is not None:
                row += ["%.6g" % float(perm[k][i])
                        for k in ("p", "q_bh", "p_maxT")]
            f.write("\t".join(row) + "\n")
    return out


def write_stability(result_name: str, genes: Sequence[str],
                    summary: dict) -> str:
    """<name>_stability.txt from stability.summarize: one tab-separated row
    per gene, in gene order. Columns GeneSymbol, Lgroup (replica 0's),
    LgroupMode, LgroupAgreement (%.4f), Selected (replicas whose biomarker
    list holds the gene), Frequency (Selected / R, %.4f), MeanGeneScore
    (%.6f, NA if no replica defines one)."""
    out = result_name + "_stability.txt"
    mgs = np.asarray(summary["mean_gene_score"], dtype=np.float64)
    with open(out, "w") as f:
        f.write("GeneSymbol\tLgroup\tLgroupMode\tLgroupAgreement\tSelected\t"
                "Frequency\tMeanGeneScore\n")
        for i, gene in enumerate(genes):
            f.write("%s\t%d\t%d\t%.4f\t%d\t%.4f\t%s\n" % (
                gene, int(summary["lgroup"][i]),
                int(summary["lgroup_mode"][i]),
                float(summary["lgroup_agreement"][i]),
                int(summary["selected"][i]), float(summary["frequency"][i]),
                "NA" if np.isnan(mgs[i]) else "%.6f" % mgs[i]))
    return out


def write_consensus(result_name: str, genes: Sequence[str],
                    summary: dict) -> str:
    """<name>_consensus_biomarkers.txt: the consensus genes of
    stability.summarize, most stable first, in the biomarker file format."""
    return write_biomarkers(result_name + "_consensus",
                            [str(genes[int(i)]) for i in summary["consensus"]])


def write_neighbors(result_name: str, genes: Sequence[str],
                    queries: Sequence[int], idx: np.ndarray, sim: np.ndarray,
                    lgroup_idx: Sequence[int],
                    biomarkers: Iterable[str]) -> str:
    """<name>_neighbors.txt: for every query gene (row index into genes, in
    the given order) its nearest genes from neighbors.nearest_genes (idx,
    sim [Q, K]), best first. Columns GeneSymbol, Rank (1..K), Neighbor,
    Cosine (%.6f), NeighborLgroup, NeighborBiomarker (0/1). Missing
    neighbours (idx == -1) are omitted."""
    out = result_name + "_neighbors.txt"
    bio = set(biomarkers)
    with open(out, "w") as f:
        f.write("GeneSymbol\tRank\tNeighbor\tCosine\tNeighborLgroup\t"
                "NeighborBiomarker\n")
        for q, row_i, row_s in zip(queries, idx, sim):
            for rank, (g, s) in enumerate(zip(row_i, row_s), start=1):
                if g < 0:
                    continue
                name = str(genes[int(g)])
                f.write("%s\t%d\t%s\t%.6f\t%d\t%d\n"
                        % (genes[int(q)], rank, name, float(s),
                           int(lgroup_idx[int(g)]), int(name in bio)))
    return out
