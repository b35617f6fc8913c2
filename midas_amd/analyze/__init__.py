"""The analysis commands over one `merge_midas.py snps` directory: snp_diversity.py (diversity.py) and call_consensus.py
(consensus.py), both on the device scan of snps_freq.txt / snps_depth.txt (midas_sites_scan)."""
