"""Records what foreign HDF5 readers return on the files tests/test_io_abi.py writes (and on the committed encoder file):

    python tests/golden/record_foreign_readers.py --h5py-python <a python with h5py> --h5dump <h5dump executable>

-> tests/golden/foreign_readers.json and tests/golden/h5py_conv2d_1_kernel.npy.  libsrcfd's HDF5 writer is deterministic, so
the tests write the same files again and compare their sha256 with the record: equal bytes are the files the readers accepted.
Re-record after a change to the writer (the tests say so by a sha256 mismatch).
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path[:0] = [os.path.dirname(TESTS), TESTS]

import srcfd_amd as srcfd                      # noqa: E402
from conftest import ENCODER_H5                 # noqa: E402
from oracle import sr_oracle as oracle          # noqa: E402
from test_io_abi import write_round_trip_file   # noqa: E402


def sha256(path):
    with open(path, "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()


def h5py_json(py, code, *args):
    return json.loads(subprocess.check_output([py, "-c", "import h5py,json,sys,numpy as np\n" + code] + list(args), text=True))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--h5py-python", required=True)
    ap.add_argument("--h5dump", required=True)
    a = ap.parse_args()
    py = a.h5py_python
    with tempfile.TemporaryDirectory() as tmp:
        kernel = os.path.join(HERE, "h5py_conv2d_1_kernel.npy")
        subprocess.check_call([py, "-c", "import h5py,numpy as np,sys;f=h5py.File(sys.argv[1],'r');"
                               "np.save(sys.argv[2], f['model_weights/conv2d_1/conv2d_1/kernel'][...])", ENCODER_H5, kernel])
        rt = os.path.join(tmp, "rt.h5")
        write_round_trip_file(srcfd, rt)
        dump = subprocess.check_output([a.h5dump, "-d", "/many/d17", rt], text=True)
        rt_h5py = h5py_json(py, "f=h5py.File(sys.argv[1],'r')\nprint(json.dumps({'backend': str(f.attrs['backend']), "
                            "'layer_names': [str(s) for s in f['model_weights'].attrs['layer_names']], 'ints_2_3': int(f['ints'][2,3]), "
                            "'many_len': len(f['many']), 'nx': np.asarray(f['Re400_mesh10x10'].attrs['nx']).ravel().tolist()}))", rt)
        enc_w = srcfd.SRModel.load_h5(ENCODER_H5, None, device=-1).weights()
        dec_w = oracle.synthetic_decoder(1)
        dec = os.path.join(tmp, "dec.h5")
        srcfd.SRModel.from_weights(None, dec_w, device=-1).save_h5(None, dec)
        dec_h5py = h5py_json(py, "f=h5py.File(sys.argv[1],'r');c=json.loads(f.attrs['model_config'])\n"
                             "print(json.dumps({'class_name': c['class_name'], 'layers': len(c['config']['layers']), "
                             "'convT0_kernel_shape': list(f['model_weights/conv2d_transpose/conv2d_transpose/kernel'].shape)}))", dec)
        sup = os.path.join(tmp, "superres.h5")
        srcfd.SRModel.from_weights(enc_w, dec_w, device=-1).save_superres_h5(sup)
        sup_h5py = h5py_json(py, "f=h5py.File(sys.argv[1],'r');c=json.loads(f.attrs['model_config'])\n"
                             "print(json.dumps({'class_name': c['class_name'], 'first_config_key': sorted(c['config'])[0], "
                             "'dense_1_kernel_shape': list(f['model_weights/decoder_400/dense_1/kernel'].shape)}))", sup)
        readers = subprocess.check_output([py, "-c", "import h5py;print('h5py', h5py.__version__, 'HDF5', h5py.version.hdf5_version)"],
                                          text=True).strip() + "; " + subprocess.check_output([a.h5dump, "--version"], text=True).strip()
        rec = {"readers": readers, "encoder_h5_sha256": sha256(ENCODER_H5),
               "round_trip": {"sha256": sha256(rt), "h5dump_many_d17": [ln.strip() for ln in dump.splitlines() if "(0):" in ln][0], "h5py": rt_h5py},
               "decoder": {"sha256": sha256(dec), "h5py": dec_h5py},
               "superres": {"sha256": sha256(sup), "h5py": sup_h5py}}
    with open(os.path.join(HERE, "foreign_readers.json"), "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
