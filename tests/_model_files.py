"""TEST INFRASTRUCTURE ONLY: the input files the model surface reads (soil table, forcing CSV) and a config over them."""
import os


def write_soil_dat(path, rows=18):
    from lgar_py_amd import data as D
    te = {12: 0.4513, 13: 0.4773, 14: 0.4617}
    tr = {12: 0.0648, 13: 0.0831, 14: 0.0668}
    with open(path, "w") as f:
        f.write("Texture\t        theta_r\ttheta_e\talpha(cm^-1)\tn\tm\tKs(cm/h)\n")
        for i in range(rows):
            a, n, k = D.VG_TABLE[i]
            f.write('"T-%d"  \t\t%g \t%g\t%g \t%g\t%g\t%g\n' % (i, tr.get(i, 0.05), te.get(i, 0.4), a, n, 1 - 1 / n, k))
    return path


def write_forcing(path, x_cm_per_h, hash_header=False, step_min=60):
    with open(path, "w") as f:
        f.write(("#" if hash_header else "") + "Time,P(mm/h),PET(mm/h)\n")
        for i, (p, e) in enumerate(x_cm_per_h):
            f.write("2016-10-01 %02d:%02d:00,%r,%r\n" % ((i * step_min) // 60 % 24, (i * step_min) % 60, float(p) * 10.0, float(e) * 10.0))
        if hash_header:
            f.write("\n\n")
    return path


def model_cfg(tmp_path, g, data="Phillipsburg", models="shorter_subcycle", n=300, **over):
    from lgar_py_amd import config
    os.makedirs(tmp_path / "data", exist_ok=True)
    soil = write_soil_dat(str(tmp_path / "data" / "vG_default_params.dat"))
    step = 60 if models == "shorter_subcycle" else 5
    forcing = write_forcing(str(tmp_path / "data" / "forcing.csv"), g["forcing"][:n], step_min=step)
    ov = {"data.forcing_file": forcing, "data.soil_params_file": soil, "models.endtime": n * step / 60.0}
    ov.update(over)
    return config.load_config(data=data, models=models, cwd=str(tmp_path), overrides=ov)
