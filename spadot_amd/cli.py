"""Command line of the package: mirror of the reference's SpaDOT/cli.py.

    python -m spadot_amd preprocess -i COUNTS [-o DIR] [--prefix preprocessed_] [--no_feature_selection]
                                    [--gene_clusters kmeans|louvain] [--device cuda:0]
    python -m spadot_amd train   -i DATA [-o DIR] [--prefix P] [--config YAML] [--device cuda:0] [--save_model]
    python -m spadot_amd analyze -i LATENT [-o DIR] [--prefix P] [--n_clusters 5,7,7,6] [--device cuda:0] [--write_tmaps]
                                 [--lineage] [--criterion elbow|silhouette|bic] [--method kmeans|gmm]
    python -m spadot_amd markers -i COUNTS --domains CSV [-o DIR] [--prefix P] [--top 100] [--device cuda:0]
    python -m spadot_amd score   -i LATENT --domains CSV [-o DIR] [--prefix P] [--device cuda:0]
    python -m spadot_amd trends  -i COUNTS [--trajectories NPZ] [--fates NPZ] [-o DIR] [--prefix P] [--top 100] [--device cuda:0]
    python -m spadot_amd neighbors --domains CSV [-o DIR] [--prefix P] [--k 6] [--n_perms 1000] [--seed 0] [--device cuda:0]
    python -m spadot_amd cooccurrence --domains CSV [-o DIR] [--prefix P] [--bins 50] [--radius R] [--ring] [--n_perms 0]
                                      [--seed 0] [--alpha 0.05] [--device cuda:0]
    python -m spadot_amd autocorr -i COUNTS [-o DIR] [--prefix P] [--k 6] [--n_perms 100] [--seed 0] [--top 100] [--device cuda:0]
    python -m spadot_amd hotspots -i COUNTS [-o DIR] [--prefix P] [--k 6] [--n_perms 999] [--seed 0] [--genes A,B | FILE] [--top 50]
                                  [--alpha 0.05] [--fdr] [--domains CSV] [--device cuda:0]
    python -m spadot_amd modules -i COUNTS [-o DIR] [--prefix P] [--k 6] [--n_perms 100] [--seed 0] [--genes A,B | FILE] [--top 100]
                                 [--min_sim 0.15] [--min_genes 2] [--alpha 0.05] [--top_pairs 0] [--device cuda:0]
    python -m spadot_amd ligrec  -i COUNTS --domains CSV --interactions CSV [-o DIR] [--prefix P] [--n_perms 1000] [--seed 0]
                                 [--threshold 0.1] [--top 100] [--device cuda:0]
    python -m spadot_amd ripley --domains CSV [-o DIR] [--prefix P] [--bins 50] [--radius R] [--n_sim 99] [--n_probes 1000]
                                [--null labels|csr] [--mode L,G,F] [--window hull|box] [--alpha 0.05] [--seed 0] [--device cuda:0]
    python -m spadot_amd correlogram -i COUNTS [-o DIR] [--prefix P] [--genes A,B | FILE] [--top 50] [--bins 12 | --radii r1,r2,..]
                                     [--n_perms 0] [--alpha 0.05] [--seed 0] [--device cuda:0]
    python -m spadot_amd embed   -i LATENT [--domains CSV] [-o DIR] [--prefix P] [--perplexity 30] [--n_iter 1000] [--early 250]
                                 [--learning_rate LR] [--per_timepoint] [--device cuda:0]
    python -m spadot_amd sepal   -i COUNTS [-o DIR] [--prefix P] [--genes A,B | FILE] [--k 6] [--dt 0.1] [--thresh 1e-8]
                                 [--n_iter 30000] [--device cuda:0]
    python -m spadot_amd territories --domains CSV [-o DIR] [--prefix P] [--k 6] [--n_perms 1000] [--seed 0] [--min_size 0]
                                     [--alpha 0.05] [--device cuda:0]
    python -m spadot_amd centrality --domains CSV [-o DIR] [--prefix P] [--k 6] [--n_perms 200] [--seed 0] [--spots]
                                    [--device cuda:0]

`preprocess` runs SPARK-X feature selection and the scaling on the device (spadot_amd.preprocess).  The balancing rule's gene
clusters come from K-means by default; `--gene_clusters louvain` clusters SCTransform Pearson residuals with Louvain as the
reference does (spadot_amd.sctransform).  `analyze --lineage` keeps the spot-level plans of all consecutive pairs on the
device and chains them: long-range transition tables, the trajectories of every domain and the fates of every spot
(spadot_amd.lineage).  `markers` tests every gene against every domain of `analyze`'s domains.csv with a Wilcoxon
rank-sum test on the device (spadot_amd.markers).  `score` gives every spot of `analyze`'s domains.csv its silhouette
coefficient in the latent space and every domain and time point the mean; `analyze --criterion silhouette` picks the adaptive
mode's k by the largest silhouette score instead of the elbow rule (spadot_amd.silhouette).  `trends` reads the
trajectories.npz and / or fates.npz of `analyze --lineage` against the counts: the weighted mean expression of every gene along
every domain's trajectory, and the correlation of every gene with every fate (spadot_amd.trends).  `analyze --method
gmm` refines every K-means labeling into a full-covariance Gaussian mixture on the device: elongated domains, a membership
probability per spot (memberships.npz, which `trends --trajectories` reads as soft domains) and, with `--criterion bic`, the k of
the smallest BIC (spadot_amd.gmm).  `neighbors` reads the spots' pixel coordinates in `analyze`'s domains.csv: on the
k-nearest-neighbour graph of every time point, the neighbourhood-enrichment permutation test of every ordered pair of domains
(counts, z-scores, empirical p-values), the share of every domain's neighbours per domain and of every spot's neighbours in its
own domain (spadot_amd.neighbors).  `cooccurrence` reads the same table: for every time point, every ordered pair of
domains and a ladder of radii up to a quarter of the tissue's diagonal (or `--radius`), the number of pairs of spots within that
distance and the co-occurrence ratio, which tells how far an association reaches; `--ring` takes the pairs between consecutive
radii instead of those within each (spadot_amd.cooccurrence); with `--n_perms S` the counts of every pair are also
tested against S random relabelings of the spots: an envelope per radius, pointwise and global p-values, and a verdict `attract`,
`avoid` or `independent` per pair of domains -- a verdict on the joint labelling, not on an interaction.  `autocorr` reads the counts and their coordinates: on the
k-nearest-neighbour graph of every time point, Moran's I and Geary's C of every gene with z-scores and p-values under the analytic
(normality) null and under random relabelings of the spots: which genes are spatially structured inside a time point, how
strongly, and with which sign (spadot_amd.autocorr).  `hotspots` reads the same counts and asks WHERE: local Moran's I
of every spot for the genes of `--genes` (default: the `--top` genes by Moran's I of every time point), with the quadrant of every
spot (high-high, low-low or an outlier) and a p-value under conditional permutation; `--domains` also counts the hot and cold
spots of every gene per domain (spadot_amd.hotspots).  `modules` reads the same counts and asks WHICH of those genes go
together: the bivariate Moran's I of every pair of the selected genes with a p-value under random relabelings, the spatial gene
modules that average linkage cuts out of it, a score of every module in every spot and the overlap of the modules of consecutive
time points (spadot_amd.modules).  `ligrec` reads the counts, the domains table and a csv of
ligand-receptor pairs (header `source,target`, gene names): for every time point, every pair and every ordered pair of domains, the
mean expression of the ligand in the one domain and of the receptor in the other, with a p-value under random relabelings of the
spots: which domains signal to which, and through which pair (spadot_amd.ligrec).  `ripley` reads the domains table and
looks at every domain on its own: Ripley's L (pairs of its spots by radius), G (the distance from a spot to the nearest spot of
its domain) and F (the distance from random probe points to the domain) over the radii of `cooccurrence`, each against an
envelope of `--n_sim` simulated patterns of the same size -- by default the domain's label dealt out at random over the spots
(`--null labels`, the right null on a lattice of spots), or points uniform in the window (`--null csr`, squidpy's) -- with
pointwise p-values, a global envelope test per domain and a verdict `clustered`, `dispersed` or `random` (spadot_amd.ripley,
DESIGN 7n).  `correlogram` reads the counts of `autocorr` and asks HOW FAR the structure of a gene reaches: Moran's I and the
semivariance of every selected gene over the pairs of spots in successive distance bands, and the range, the distance at which the
autocorrelation stops (spadot_amd.correlogram).  `embed` reads the latents and draws the map a user looks at first: a
t-SNE of all time points together (or of every time point on its own with `--per_timepoint`) with sklearn's objective and
optimiser and the repulsion summed exactly over all pairs in fp64, bitwise repeatable; with `--domains` the table and the plot
carry the domain of every spot (spadot_amd.embed).  `sepal` reads the counts of `autocorr` and asks HOW LARGE the pattern
of a gene is: the expression of every gene of `--genes` (default: all) diffuses over the k-nearest-neighbour graph of every time
point, and the time until its entropy stops changing is the score of the gene -- a broad gradient takes long, fine-grained texture
and noise are flat almost at once; a ranking by the scale of a pattern beside SPARK-X and Moran's I (spadot_amd.sepal, DESIGN
7q).  `territories` reads the domains table and looks at the map itself: the connected pieces of every domain on the
k-nearest-neighbour graph of every time point (how many, the largest, the stray single spots, a contiguity between 0 and 1),
each against `--n_perms` random relabelings, the territory of every spot and whether it lies on a border; with `--min_size S`
every piece of fewer than S spots is handed to the domain it touches most and the cleaned map is written as
refined_domains.csv, which every `--domains` stage reads (spadot_amd.territories).  `centrality` reads the domains
table and measures how far apart things are along the tissue, in hops on the k-nearest-neighbour graph of every time point:
per domain the group closeness and group degree centrality of squidpy's `gr.centrality_scores` and its eccentricity, per
ordered pair of domains the mean number of hops from a spot of one to the nearest spot of the other, each against `--n_perms`
random relabelings, per spot the hops to every domain and its depth inside its own; with `--spots` also the closeness and
eccentricity of every single spot, the diameter, the radius and the centre of the tissue (spadot_amd.centrality)."""
import argparse
import os
import sys


def _n_clusters(s):
    return [int(item) for item in s.split(",")]


def build_parser():
    parser = argparse.ArgumentParser(
        description="SpaDOT on the MI355X: optimal transport modeling uncovers spatial domain dynamics in spatiotemporal "
                    "transcriptomics.", prog="spadot_amd")
    sub = parser.add_subparsers(help="sub-command help.", dest="cmd_choice")

    pre = sub.add_parser("preprocess", help="Preprocess raw counts: SPARK-X feature selection, normalisation and scaling.")
    pre.add_argument("-i", "--data", dest="data", type=str,
                     help="Raw counts: an .h5ad (needs anndata) or .npz with timepoint, spatial and the counts.")
    pre.add_argument("-o", "--output_dir", dest="output_dir", type=str,
                     help="Output directory. Default: the same as where the data locates.")
    pre.add_argument("--prefix", dest="prefix", type=str, default="preprocessed_",
                     help="Prefix of the preprocessed data file. Default: preprocessed_")
    pre.add_argument("--feature_selection", dest="feature_selection", default=True, action="store_true",
                     help="Select spatially variable genes with SPARK-X (the default).")
    pre.add_argument("--no_feature_selection", dest="feature_selection", action="store_false",
                     help="Keep all genes: only normalise, log-transform and scale.")
    pre.add_argument("--gene_clusters", dest="gene_clusters", choices=("kmeans", "louvain"), default="kmeans",
                     help="Gene clusters of the balancing rule: K-means on log-normalised counts, or Louvain on SCTransform "
                          "residuals as the reference. Default: kmeans")
    pre.add_argument("--device", dest="device", type=str, default="cuda:0", help="Device to use. Default: cuda:0")

    tr = sub.add_parser("train", help="Train a SpaDOT model.")
    tr.add_argument("-i", "--data", dest="data", type=str,
                    help="An .h5ad (needs anndata) or .npz file containing time point information and spatial coordinates.")
    tr.add_argument("-o", "--output_dir", dest="output_dir", type=str,
                    help="Output directory to store latent representations. Default: the same as where the data locates.")
    tr.add_argument("--prefix", dest="prefix", type=str, default="", help="Prefix for output latent representations. Default: ''")
    tr.add_argument("--config", dest="config", type=str, help="Path to the config file, in a yaml format.")
    tr.add_argument("--device", dest="device", type=str, default="cuda:0", help="Device to use for training. Default: cuda:0")
    tr.add_argument("--save_model", dest="save_model", default=False, action="store_true",
                    help="Whether saving the trained model (SpaDOT_model.pth in the output_dir).")

    an = sub.add_parser("analyze", help="Analyze the latent representations generated by the SpaDOT model.")
    an.add_argument("-i", "--data", dest="data", type=str, required=True,
                    help="The latent representations: latent.npz (or latent.h5ad, needs anndata) written by train.")
    an.add_argument("-o", "--output_dir", dest="output_dir", type=str,
                    help="Output directory to store analyses results. Default: the same as where the data locates.")
    an.add_argument("--prefix", dest="prefix", type=str, default="", help="Prefix for output analyses results. Default: ''")
    an.add_argument("--n_clusters", dest="n_clusters", type=_n_clusters,
                    help="A comma-separated list of integers, the number of clusters of each time point. "
                         "Default: chosen per time point by the adaptive elbow rule over k = 4 .. 20.")
    an.add_argument("--device", dest="device", type=str, default="cuda:0", help="Device to use. Default: cuda:0")
    an.add_argument("--write_tmaps", dest="write_tmaps", default=False, action="store_true",
                    help="Also write the spot-level transport maps under OT/.")
    an.add_argument("--lineage", dest="lineage", default=False, action="store_true",
                    help="Also chain the transport plans across time points: transition tables between non-consecutive time "
                         "points, trajectories.npz (ancestors and descendants of every domain) and fates.npz (per spot, the "
                         "share of its mass that ends in each domain of the last time point).")
    an.add_argument("--criterion", dest="criterion", choices=("elbow", "silhouette", "bic"), default="elbow",
                    help="How the adaptive mode picks the number of clusters: the reference's elbow rule on the WSS curve, "
                         "the largest silhouette score of the fits (also writes {tp}_silhouette.csv), or the smallest BIC of the "
                         "Gaussian mixtures (needs --method gmm; writes {tp}_BIC.csv). Not with --n_clusters. Default: elbow")
    an.add_argument("--method", dest="method", choices=("kmeans", "gmm"), default="kmeans",
                    help="What a domain is: a K-means cluster, or a component of a full-covariance Gaussian mixture started "
                         "from the K-means labels (elongated domains; also writes memberships.npz, the membership probability of "
                         "every spot in every domain, and gmm.npz). The adaptive mode of gmm needs --criterion bic or silhouette. "
                         "Default: kmeans")

    mk = sub.add_parser("markers", help="Marker genes of the spatial domains: per-domain Wilcoxon rank-sum tests of every gene.")
    mk.add_argument("-i", "--data", dest="data", type=str, required=True,
                    help="The counts: the .npz written by preprocess (its raw counts of the selected genes), or raw counts as "
                         "preprocess reads them (.npz or .h5ad).")
    mk.add_argument("--domains", dest="domains", type=str, required=True,
                    help="The domains.csv written by analyze: row, timepoint, kmeans.")
    mk.add_argument("-o", "--output_dir", dest="output_dir", type=str,
                    help="Output directory. Default: the same as where the data locates.")
    mk.add_argument("--prefix", dest="prefix", type=str, default="", help="Prefix for the marker tables. Default: ''")
    mk.add_argument("--top", dest="top", type=int, default=100,
                    help="Genes listed per domain in the csv tables, by descending score; 0 lists all. Default: 100")
    mk.add_argument("--device", dest="device", type=str, default="cuda:0", help="Device to use. Default: cuda:0")

    sc = sub.add_parser("score", help="Silhouette coefficients of the spatial domains in the latent space: per spot, per domain "
                                      "and per time point.")
    sc.add_argument("-i", "--data", dest="data", type=str, required=True,
                    help="The latent representations: latent.npz (or latent.h5ad, needs anndata) written by train.")
    sc.add_argument("--domains", dest="domains", type=str, required=True,
                    help="The domains.csv written by analyze: row, timepoint, kmeans.")
    sc.add_argument("-o", "--output_dir", dest="output_dir", type=str,
                    help="Output directory. Default: the same as where the data locates.")
    sc.add_argument("--prefix", dest="prefix", type=str, default="", help="Prefix for the silhouette tables. Default: ''")
    sc.add_argument("--device", dest="device", type=str, default="cuda:0", help="Device to use. Default: cuda:0")

    tn = sub.add_parser("trends", help="Gene trends along the trajectories of the domains and the genes that go with each fate.")
    tn.add_argument("-i", "--data", dest="data", type=str, required=True,
                    help="The counts: the .npz written by preprocess (its raw counts of the selected genes), or raw counts as "
                         "preprocess reads them (.npz or .h5ad).")
    tn.add_argument("--trajectories", dest="trajectories", type=str,
                    help="The trajectories.npz written by analyze --lineage: weighted mean expression of every gene along every "
                         "trajectory.")
    tn.add_argument("--fates", dest="fates", type=str,
                    help="The fates.npz written by analyze --lineage: correlation of every gene with every fate.")
    tn.add_argument("-o", "--output_dir", dest="output_dir", type=str,
                    help="Output directory. Default: the same as where the data locates.")
    tn.add_argument("--prefix", dest="prefix", type=str, default="", help="Prefix for the trend tables. Default: ''")
    tn.add_argument("--top", dest="top", type=int, default=100,
                    help="Genes listed per trajectory and per fate in the csv tables; 0 lists all. Default: 100")
    tn.add_argument("--device", dest="device", type=str, default="cuda:0", help="Device to use. Default: cuda:0")

    nb = sub.add_parser("neighbors", help="Neighbourhood enrichment of the spatial domains: which domains border which, on the "
                                          "k-nearest-neighbour graph of every time point.")
    nb.add_argument("--domains", dest="domains", type=str, required=True,
                    help="The domains.csv written by analyze: row, timepoint, kmeans, pixel_x, pixel_y.")
    nb.add_argument("-o", "--output_dir", dest="output_dir", type=str,
                    help="Output directory. Default: the same as where the domains table locates.")
    nb.add_argument("--prefix", dest="prefix", type=str, default="", help="Prefix for the enrichment tables. Default: ''")
    nb.add_argument("--k", dest="k", type=int, default=6, help="Spatial neighbours per spot. Default: 6")
    nb.add_argument("--n_perms", dest="n_perms", type=int, default=1000,
                    help="Random relabelings (domain sizes kept) behind the z-scores and p-values. Default: 1000")
    nb.add_argument("--seed", dest="seed", type=int, default=0, help="Seed of the relabelings. Default: 0")
    nb.add_argument("--device", dest="device", type=str, default="cuda:0", help="Device to use. Default: cuda:0")

    te = sub.add_parser("territories", help="The connected pieces of every spatial domain on the k-nearest-neighbour graph of "
                                            "every time point: one piece or forty, which spots are strays, and a map "
                                            "cleaned of them.")
    te.add_argument("--domains", dest="domains", type=str, required=True,
                    help="The domains.csv written by analyze: row, timepoint, kmeans, pixel_x, pixel_y.")
    te.add_argument("-o", "--output_dir", dest="output_dir", type=str,
                    help="Output directory. Default: the same as where the domains table locates.")
    te.add_argument("--prefix", dest="prefix", type=str, default="", help="Prefix for the territory tables. Default: ''")
    te.add_argument("--k", dest="k", type=int, default=6, help="Spatial neighbours per spot. Default: 6")
    te.add_argument("--n_perms", dest="n_perms", type=int, default=1000,
                    help="Random relabelings (domain sizes kept) behind the z-scores and p-values, 0 to 9999; 0: no test. "
                         "Default: 1000")
    te.add_argument("--seed", dest="seed", type=int, default=0, help="Seed of the relabelings. Default: 0")
    te.add_argument("--min_size", dest="min_size", type=int, default=0,
                    help="Hand every territory of fewer spots to the domain it touches most and write refined_domains.csv; 0: "
                         "off, otherwise at least 2. Default: 0")
    te.add_argument("--alpha", dest="alpha", type=float, default=0.05,
                    help="Level of the adjusted p-value below which a domain is called contiguous or fragmented. Default: 0.05")
    te.add_argument("--device", dest="device", type=str, default="cuda:0", help="Device to use. Default: cuda:0")

    ce = sub.add_parser("centrality", help="Hop distances along the tissue: group closeness and degree centrality of every "
                                           "spatial domain, the mean hops between every pair of domains, and how deep inside "
                                           "its domain every spot sits.")
    ce.add_argument("--domains", dest="domains", type=str, required=True,
                    help="The domains.csv written by analyze: row, timepoint, kmeans, pixel_x, pixel_y.")
    ce.add_argument("-o", "--output_dir", dest="output_dir", type=str,
                    help="Output directory. Default: the same as where the domains table locates.")
    ce.add_argument("--prefix", dest="prefix", type=str, default="", help="Prefix for the centrality tables. Default: ''")
    ce.add_argument("--k", dest="k", type=int, default=6, help="Spatial neighbours per spot. Default: 6")
    ce.add_argument("--n_perms", dest="n_perms", type=int, default=200,
                    help="Random relabelings (domain sizes kept) behind the z-scores and p-values, 0 to 9999; 0: no null. "
                         "Default: 200")
    ce.add_argument("--seed", dest="seed", type=int, default=0, help="Seed of the relabelings. Default: 0")
    ce.add_argument("--spots", dest="spots", action="store_true",
                    help="Also a breadth-first search from every single spot: its closeness and eccentricity, the diameter, "
                         "the radius and the centre spots of every time point.")
    ce.add_argument("--device", dest="device", type=str, default="cuda:0", help="Device to use. Default: cuda:0")

    co = sub.add_parser("cooccurrence", help="Co-occurrence of the spatial domains by distance: for every pair of domains, how "
                                             "many pairs of spots lie within each radius and the ratio to what the "
                                             "domains' sizes alone would give.")
    co.add_argument("--domains", dest="domains", type=str, required=True,
                    help="The domains.csv written by analyze: row, timepoint, kmeans, pixel_x, pixel_y.")
    co.add_argument("-o", "--output_dir", dest="output_dir", type=str,
                    help="Output directory. Default: the same as where the domains table locates.")
    co.add_argument("--prefix", dest="prefix", type=str, default="", help="Prefix for the co-occurrence tables. Default: ''")
    co.add_argument("--bins", dest="bins", type=int, default=50, help="Radii per time point, 1 to 64. Default: 50")
    co.add_argument("--radius", dest="radius", type=float,
                    help="The largest radius, in the units of pixel_x / pixel_y. Default: per time point, a quarter of the "
                         "diagonal of the spots' bounding box.")
    co.add_argument("--ring", dest="ring", default=False, action="store_true",
                    help="Ratios of the pairs between consecutive radii (annuli) instead of within each radius (discs).")
    co.add_argument("--n_perms", dest="n_perms", type=int, default=0,
                    help="Random relabelings of the spots per time point, 0 to 9999: with 1 or more, the counts of every pair of "
                         "domains are tested against them (envelope, p-values, a verdict attract / avoid / independent per "
                         "pair). Default: 0, no test")
    co.add_argument("--seed", dest="seed", type=int, default=0, help="Seed of the relabelings. Default: 0")
    co.add_argument("--alpha", dest="alpha", type=float, default=0.05,
                    help="Level of the adjusted global p-value below which a pair is called attract or avoid. Default: 0.05")
    co.add_argument("--device", dest="device", type=str, default="cuda:0", help="Device to use. Default: cuda:0")

    rp = sub.add_parser("ripley", help="Ripley's L, G and F of every spatial domain on its own, against a Monte-Carlo envelope: "
                                       "one territory, scattered islands, or no different from chance, and at which scale.")
    rp.add_argument("--domains", dest="domains", type=str, required=True,
                    help="The domains.csv written by analyze: row, timepoint, kmeans, pixel_x, pixel_y.")
    rp.add_argument("-o", "--output_dir", dest="output_dir", type=str,
                    help="Output directory. Default: the same as where the domains table locates.")
    rp.add_argument("--prefix", dest="prefix", type=str, default="", help="Prefix for the ripley tables. Default: ''")
    rp.add_argument("--bins", dest="bins", type=int, default=50, help="Radii per time point, 1 to 64. Default: 50")
    rp.add_argument("--radius", dest="radius", type=float,
                    help="The largest radius, in the units of pixel_x / pixel_y. Default: per time point, a quarter of the "
                         "diagonal of the spots' bounding box.")
    rp.add_argument("--n_sim", dest="n_sim", type=int, default=99, help="Simulated patterns per domain, 1 to 9999. Default: 99")
    rp.add_argument("--n_probes", dest="n_probes", type=int, default=1000,
                    help="Probe points per time point behind F, 1 to 1048576. Default: 1000")
    rp.add_argument("--null", dest="null", type=str, default="labels", choices=["labels", "csr"],
                    help="The simulated patterns: the domain's label dealt out at random over the spots (labels), or points "
                         "uniform in the window (csr). Default: labels")
    rp.add_argument("--mode", dest="mode", type=str, default="L,G,F", help="The statistics to count, of L, G and F. Default: L,G,F")
    rp.add_argument("--window", dest="window", type=str, default="hull", choices=["hull", "box"],
                    help="The window: the convex hull of a time point's spots, or their bounding box. Default: hull")
    rp.add_argument("--alpha", dest="alpha", type=float, default=0.05,
                    help="Level of the global envelope test behind the `pattern` column. Default: 0.05")
    rp.add_argument("--seed", dest="seed", type=int, default=0, help="Seed of the simulations and the probe points. Default: 0")
    rp.add_argument("--device", dest="device", type=str, default="cuda:0", help="Device to use. Default: cuda:0")

    ac = sub.add_parser("autocorr", help="Spatial autocorrelation of every gene inside every time point: Moran's I and Geary's C "
                                         "on the k-nearest-neighbour graph, with an analytic and a permutation null.")
    ac.add_argument("-i", "--data", dest="data", type=str, required=True,
                    help="The counts: the .npz written by preprocess (its raw counts of the selected genes), or raw counts as "
                         "preprocess reads them (.npz or .h5ad).")
    ac.add_argument("-o", "--output_dir", dest="output_dir", type=str,
                    help="Output directory. Default: the same as where the data locates.")
    ac.add_argument("--prefix", dest="prefix", type=str, default="", help="Prefix for the autocorrelation tables. Default: ''")
    ac.add_argument("--k", dest="k", type=int, default=6, help="Spatial neighbours per spot. Default: 6")
    ac.add_argument("--n_perms", dest="n_perms", type=int, default=100,
                    help="Random relabelings of the spots behind z_sim and p_sim; 0 leaves the analytic null alone. Default: 100")
    ac.add_argument("--seed", dest="seed", type=int, default=0, help="Seed of the relabelings. Default: 0")
    ac.add_argument("--top", dest="top", type=int, default=100,
                    help="Genes listed per time point in the csv tables, by descending I; 0 lists all. Default: 100")
    ac.add_argument("--device", dest="device", type=str, default="cuda:0", help="Device to use. Default: cuda:0")

    hs = sub.add_parser("hotspots", help="Where a gene is spatially structured: local Moran's I of every spot on the "
                                         "k-nearest-neighbour graph of every time point, with quadrants and a conditional "
                                         "permutation null.")
    hs.add_argument("-i", "--data", dest="data", type=str, required=True,
                    help="The counts: the .npz written by preprocess (its raw counts of the selected genes), or raw counts as "
                         "preprocess reads them (.npz or .h5ad).")
    hs.add_argument("-o", "--output_dir", dest="output_dir", type=str,
                    help="Output directory. Default: the same as where the data locates.")
    hs.add_argument("--prefix", dest="prefix", type=str, default="", help="Prefix for the hot-spot tables. Default: ''")
    hs.add_argument("--k", dest="k", type=int, default=6, help="Spatial neighbours per spot. Default: 6")
    hs.add_argument("--n_perms", dest="n_perms", type=int, default=999,
                    help="Conditional relabelings of the spots behind p_sim, at least 1. Default: 999")
    hs.add_argument("--seed", dest="seed", type=int, default=0, help="Seed of the relabelings. Default: 0")
    hs.add_argument("--genes", dest="genes", type=str,
                    help="The genes to test: a comma-separated list of names, or a file with one name per line. Default: the "
                         "--top genes by Moran's I of every time point.")
    hs.add_argument("--top", dest="top", type=int, default=50,
                    help="Without --genes: the genes taken per time point by descending Moran's I (their union is tested). "
                         "Default: 50")
    hs.add_argument("--alpha", dest="alpha", type=float, default=0.05,
                    help="A spot is significant where p_sim (folded, as esda's Moran_Local) is at most this. Default: 0.05")
    hs.add_argument("--fdr", dest="fdr", default=False, action="store_true",
                    help="Compare the Benjamini-Hochberg adjusted p-value (over the spots of a gene and time point) with --alpha "
                         "instead.")
    hs.add_argument("--domains", dest="domains", type=str,
                    help="The domains.csv written by analyze: also write the significant high-high and low-low spots of every "
                         "gene per domain.")
    hs.add_argument("--device", dest="device", type=str, default="cuda:0", help="Device to use. Default: cuda:0")

    mo = sub.add_parser("modules", help="Which spatially structured genes go together: the bivariate Moran's I of every pair of "
                                        "selected genes on the k-nearest-neighbour graph of every time point, with a "
                                        "permutation null, and the spatial gene modules cut out of it.")
    mo.add_argument("-i", "--data", dest="data", type=str, required=True,
                    help="The counts: the .npz written by preprocess (its raw counts of the selected genes), or raw counts as "
                         "preprocess reads them (.npz or .h5ad).")
    mo.add_argument("-o", "--output_dir", dest="output_dir", type=str,
                    help="Output directory. Default: the same as where the data locates.")
    mo.add_argument("--prefix", dest="prefix", type=str, default="", help="Prefix for the module tables. Default: ''")
    mo.add_argument("--k", dest="k", type=int, default=6, help="Spatial neighbours per spot. Default: 6")
    mo.add_argument("--n_perms", dest="n_perms", type=int, default=100,
                    help="Random relabelings of the spots behind z_sim and p_sim, at least 1. Default: 100")
    mo.add_argument("--seed", dest="seed", type=int, default=0, help="Seed of the relabelings. Default: 0")
    mo.add_argument("--genes", dest="genes", type=str,
                    help="The genes to group: a comma-separated list of names, or a file with one name per line. Default: the "
                         "--top genes by Moran's I of every time point.")
    mo.add_argument("--top", dest="top", type=int, default=100,
                    help="Without --genes: the genes taken per time point by descending Moran's I (their union is grouped). "
                         "Default: 100")
    mo.add_argument("--min_sim", dest="min_sim", type=float, default=0.15,
                    help="Average-linkage clusters are cut where the mean bivariate Moran's I between them falls below this. "
                         "Default: 0.15")
    mo.add_argument("--min_genes", dest="min_genes", type=int, default=2,
                    help="A cluster of fewer genes is no module (label -1). Default: 2")
    mo.add_argument("--alpha", dest="alpha", type=float, default=0.05,
                    help="The pairs with a Benjamini-Hochberg adjusted p-value of at most this are counted in the summary. "
                         "Default: 0.05")
    mo.add_argument("--top_pairs", dest="top_pairs", type=int, default=0,
                    help="Pairs listed per time point in the pair tables, by descending |R|; 0 lists all. Default: 0")
    mo.add_argument("--device", dest="device", type=str, default="cuda:0", help="Device to use. Default: cuda:0")

    cg = sub.add_parser("correlogram", help="How far the spatial structure of a gene reaches: Moran's I and the semivariance of "
                                            "every selected gene over the pairs of spots in successive distance bands, and "
                                            "the range at which the autocorrelation stops.")
    cg.add_argument("-i", "--data", dest="data", type=str, required=True,
                    help="The counts: the .npz written by preprocess (its raw counts of the selected genes), or raw counts as "
                         "preprocess reads them (.npz or .h5ad).")
    cg.add_argument("-o", "--output_dir", dest="output_dir", type=str,
                    help="Output directory. Default: the same as where the data locates.")
    cg.add_argument("--prefix", dest="prefix", type=str, default="", help="Prefix for the correlogram tables. Default: ''")
    cg.add_argument("--genes", dest="genes", type=str,
                    help="The genes to test: a comma-separated list of names, or a file with one name per line. Default: the "
                         "--top genes by Moran's I of every time point.")
    cg.add_argument("--top", dest="top", type=int, default=50,
                    help="Without --genes: the genes taken per time point by descending Moran's I (their union is tested). "
                         "Default: 50")
    cg.add_argument("--bins", dest="bins", type=int, default=12, help="Distance bands per time point, 1 to 16. Default: 12")
    cg.add_argument("--radii", dest="radii", type=str,
                    help="The upper ends of the bands, in the units of the coordinates: a comma-separated increasing list of 1 "
                         "to 16 radii, for every time point. Default: --bins equal bands up to a quarter of the diagonal of "
                         "the time point's bounding box.")
    cg.add_argument("--n_perms", dest="n_perms", type=int, default=0,
                    help="Random relabelings of the spots behind z_sim and p_sim; 0 tests against the analytic null alone. "
                         "Default: 0")
    cg.add_argument("--alpha", dest="alpha", type=float, default=0.05,
                    help="The range of a gene ends at the first band whose adjusted p-value is above this (or whose Moran's I "
                         "is not above its expectation). Default: 0.05")
    cg.add_argument("--seed", dest="seed", type=int, default=0, help="Seed of the relabelings. Default: 0")
    cg.add_argument("--device", dest="device", type=str, default="cuda:0", help="Device to use. Default: cuda:0")

    em = sub.add_parser("embed", help="A two-dimensional t-SNE map of the latent space, all time points together or one map per "
                                      "time point: exact repulsion in fp64 on the device, bitwise repeatable.")
    em.add_argument("-i", "--data", dest="data", type=str, required=True,
                    help="The latent representations: latent.npz (or latent.h5ad, needs anndata) written by train.")
    em.add_argument("--domains", dest="domains", type=str,
                    help="The domains.csv written by analyze (row, timepoint, kmeans): adds the kmeans column and the second panel "
                         "of the plot.")
    em.add_argument("-o", "--output_dir", dest="output_dir", type=str,
                    help="Output directory. Default: the same as where the data locates.")
    em.add_argument("--prefix", dest="prefix", type=str, default="", help="Prefix for the embedding files. Default: ''")
    em.add_argument("--perplexity", dest="perplexity", type=float, default=30.0,
                    help="Perplexity of the input affinities, 2 to 50; every embedded set needs perplexity + 2 spots. Default: 30")
    em.add_argument("--n_iter", dest="n_iter", type=int, default=1000, help="Iterations; there is no early stop. Default: 1000")
    em.add_argument("--early", dest="early", type=int, default=250,
                    help="Iterations of the early-exaggeration phase (exaggeration 12, momentum 0.5). Default: 250")
    em.add_argument("--learning_rate", dest="learning_rate", type=float,
                    help="Learning rate. Default: max(n / 12 / 4, 50) for a set of n spots, as sklearn's 'auto'.")
    em.add_argument("--per_timepoint", dest="per_timepoint", default=False, action="store_true",
                    help="One embedding per time point (one launch for all of them) instead of one joint embedding.")
    em.add_argument("--device", dest="device", type=str, default="cuda:0", help="Device to use. Default: cuda:0")

    sp = sub.add_parser("sepal", help="How large the spatial pattern of a gene is: the time its expression takes to become "
                                      "homogeneous when it diffuses over the spatial graph of every time point.")
    sp.add_argument("-i", "--data", dest="data", type=str, required=True,
                    help="The counts: the .npz written by preprocess (its raw counts of the selected genes), or raw counts as "
                         "preprocess reads them (.npz or .h5ad).")
    sp.add_argument("-o", "--output_dir", dest="output_dir", type=str,
                    help="Output directory. Default: the same as where the data locates.")
    sp.add_argument("--prefix", dest="prefix", type=str, default="", help="Prefix for the sepal tables. Default: ''")
    sp.add_argument("--genes", dest="genes", type=str,
                    help="The genes to score: a comma-separated list of names, or a file with one name per line. Default: all.")
    sp.add_argument("--k", dest="k", type=int, default=6, help="Nearest neighbours per spot in the spatial graph. Default: 6")
    sp.add_argument("--dt", dest="dt", type=float, default=0.1,
                    help="Time step; dt n / (2 E) times the largest degree of the symmetric graph must stay below 1. Default: 0.1")
    sp.add_argument("--thresh", dest="thresh", type=float, default=1e-8,
                    help="A gene stops at the first step that changes its entropy by at most this. Default: 1e-8")
    sp.add_argument("--n_iter", dest="n_iter", type=int, default=30000,
                    help="Steps after which a gene that has not stopped is given up (it keeps the score dt * n_iter). Default: 30000")
    sp.add_argument("--device", dest="device", type=str, default="cuda:0", help="Device to use. Default: cuda:0")

    lr = sub.add_parser("ligrec", help="Ligand-receptor tests between the spatial domains of every time point: the mean expression "
                                       "of every pair between every two domains, with a permutation null.")
    lr.add_argument("-i", "--data", dest="data", type=str, required=True,
                    help="The counts: the .npz written by preprocess (its raw counts of the selected genes), or raw counts as "
                         "preprocess reads them (.npz or .h5ad).")
    lr.add_argument("--domains", dest="domains", type=str, required=True,
                    help="The domains.csv written by analyze: row, timepoint, kmeans.")
    lr.add_argument("--interactions", dest="interactions", type=str, required=True,
                    help="A csv with the header source,target: one ligand-receptor pair of gene names per row.")
    lr.add_argument("-o", "--output_dir", dest="output_dir", type=str,
                    help="Output directory. Default: the same as where the data locates.")
    lr.add_argument("--prefix", dest="prefix", type=str, default="", help="Prefix for the ligand-receptor tables. Default: ''")
    lr.add_argument("--n_perms", dest="n_perms", type=int, default=1000,
                    help="Random relabelings of the spots (domain sizes kept) behind the p-values; 0 reports the means alone. "
                         "Default: 1000")
    lr.add_argument("--seed", dest="seed", type=int, default=0, help="Seed of the relabelings. Default: 0")
    lr.add_argument("--threshold", dest="threshold", type=float, default=0.1,
                    help="Share of a domain's spots that must express a gene for its cells to be tested. Default: 0.1")
    lr.add_argument("--top", dest="top", type=int, default=100,
                    help="Cells listed per time point in the csv tables, by ascending p-value; 0 lists all. Default: 100")
    lr.add_argument("--device", dest="device", type=str, default="cuda:0", help="Device to use. Default: cuda:0")
    return parser


def parse_args(argv=None):
    args = build_parser().parse_args(argv)
    print("User input arguments: ", args)
    return args


def _exists(path):
    return bool(path) and os.path.exists(path)


def main(argv=None):
    args = parse_args(argv)
    if args.cmd_choice == "preprocess":
        if not _exists(args.data):
            print(f"SpaDOT preprocess: the data does not exist: {args.data}. Please make sure the data is correctly "
                  "specified.", file=sys.stderr)
            sys.exit(2)
        from .preprocess import preprocess
        preprocess(args)
    elif args.cmd_choice == "train":
        from .train import train
        if not _exists(args.data):
            sys.exit("The preprocessed data does not exist! Please make sure the data is correctly specified.")
        train(args)
    elif args.cmd_choice == "analyze":
        from .analyze import analyze
        if not _exists(args.data):
            sys.exit("The latent representations does not exist! Please make sure the latent representations are correctly "
                     "generated from the last step.")
        analyze(args)
    elif args.cmd_choice == "markers":
        for what, path in (("counts", args.data), ("domains table", args.domains)):
            if not _exists(path):
                print(f"SpaDOT markers: the {what} does not exist: {path}. Please make sure it is correctly specified.",
                      file=sys.stderr)
                sys.exit(2)
        from .markers import markers
        markers(args)
    elif args.cmd_choice == "score":
        for what, path in (("latent representations", args.data), ("domains table", args.domains)):
            if not _exists(path):
                print(f"SpaDOT score: the {what} does not exist: {path}. Please make sure it is correctly specified.",
                      file=sys.stderr)
                sys.exit(2)
        from .silhouette import score
        score(args)
    elif args.cmd_choice == "trends":
        named = [(w, p) for w, p in (("trajectories", args.trajectories), ("fates", args.fates)) if p]
        for what, path in [("counts", args.data)] + named:
            if not _exists(path):
                print(f"SpaDOT trends: the {what} does not exist: {path}. Please make sure it is correctly specified.",
                      file=sys.stderr)
                sys.exit(2)
        from .trends import trends
        trends(args)
    elif args.cmd_choice == "neighbors":
        if not _exists(args.domains):
            print(f"SpaDOT neighbors: the domains table does not exist: {args.domains}. Please make sure it is correctly "
                  "specified.", file=sys.stderr)
            sys.exit(2)
        from .neighbors import neighbors
        neighbors(args)
    elif args.cmd_choice == "territories":
        if not _exists(args.domains):
            print(f"SpaDOT territories: the domains table does not exist: {args.domains}. Please make sure it is correctly "
                  "specified.", file=sys.stderr)
            sys.exit(2)
        from .territories import territories_stage
        territories_stage(args)
    elif args.cmd_choice == "centrality":
        if not _exists(args.domains):
            print(f"SpaDOT centrality: the domains table does not exist: {args.domains}. Please make sure it is correctly "
                  "specified.", file=sys.stderr)
            sys.exit(2)
        from .centrality import centrality_stage
        centrality_stage(args)
    elif args.cmd_choice == "cooccurrence":
        if not _exists(args.domains):
            print(f"SpaDOT cooccurrence: the domains table does not exist: {args.domains}. Please make sure it is correctly "
                  "specified.", file=sys.stderr)
            sys.exit(2)
        from .cooccurrence import cooccur
        cooccur(args)
    elif args.cmd_choice == "ripley":
        if not _exists(args.domains):
            print(f"SpaDOT ripley: the domains table does not exist: {args.domains}. Please make sure it is correctly "
                  "specified.", file=sys.stderr)
            sys.exit(2)
        from .ripley import ripley_stage
        ripley_stage(args)
    elif args.cmd_choice == "autocorr":
        if not _exists(args.data):
            print(f"SpaDOT autocorr: the counts do not exist: {args.data}. Please make sure they are correctly specified.",
                  file=sys.stderr)
            sys.exit(2)
        from .autocorr import autocorr
        autocorr(args)
    elif args.cmd_choice == "hotspots":
        named = [("domains table", args.domains)] if args.domains else []
        for what, path in [("counts", args.data)] + named:
            if not _exists(path):
                print(f"SpaDOT hotspots: the {what} does not exist: {path}. Please make sure it is correctly specified.",
                      file=sys.stderr)
                sys.exit(2)
        from .hotspots import hotspots
        hotspots(args)
    elif args.cmd_choice == "modules":
        if not _exists(args.data):
            print(f"SpaDOT modules: the counts do not exist: {args.data}. Please make sure they are correctly specified.",
                  file=sys.stderr)
            sys.exit(2)
        from .modules import modules
        modules(args)
    elif args.cmd_choice == "correlogram":
        if not _exists(args.data):
            print(f"SpaDOT correlogram: the counts do not exist: {args.data}. Please make sure they are correctly specified.",
                  file=sys.stderr)
            sys.exit(2)
        from .correlogram import correlogram_stage
        correlogram_stage(args)
    elif args.cmd_choice == "embed":
        named = [("domains table", args.domains)] if args.domains else []
        for what, path in [("latent representations", args.data)] + named:
            if not _exists(path):
                print(f"SpaDOT embed: the {what} does not exist: {path}. Please make sure it is correctly specified.",
                      file=sys.stderr)
                sys.exit(2)
        from .embed import embed
        embed(args)
    elif args.cmd_choice == "sepal":
        if not _exists(args.data):
            print(f"SpaDOT sepal: the counts do not exist: {args.data}. Please make sure they are correctly specified.",
                  file=sys.stderr)
            sys.exit(2)
        from .sepal import sepal_stage
        sepal_stage(args)
    elif args.cmd_choice == "ligrec":
        for what, path in (("counts", args.data), ("domains table", args.domains), ("interactions table", args.interactions)):
            if not _exists(path):
                print(f"SpaDOT ligrec: the {what} does not exist: {path}. Please make sure it is correctly specified.",
                      file=sys.stderr)
                sys.exit(2)
        from .ligrec import interactions
        interactions(args)
    else:
        build_parser().print_help()
        sys.exit(2)


if __name__ == "__main__":
    main()
