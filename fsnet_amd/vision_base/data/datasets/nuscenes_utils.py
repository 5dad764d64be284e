"""The nuScenes table accessor with the reference's per-(dataroot, version) singleton
(vision_base/data/datasets/nuscenes_utils.py:1-6).  With the devkit installed, `NuScenes(...)` is the devkit's object,
as in the reference.  Without it, it is NuScenesTables: a reader of <dataroot>/<version>/*.json with what the
evaluator's export and NusceneDepthMonoDataset use and no more — get(table, token), .sample, .scene, .dataroot and
sample['data'][channel], built like the devkit's reverse index: key-frame sample_data -> calibrated_sensor -> sensor."""
import json
import os

GLOBAL_DICT = {}


class NuScenesTables(object):
    def __init__(self, version='v1.0-mini', dataroot='/data/sets/nuscenes', verbose=False, **kwargs):
        self.version, self.dataroot, self.verbose = version, dataroot, verbose
        self.table_root = os.path.join(dataroot, version)
        self._tables, self._index = {}, {}
        for sample in self.sample:
            sample['data'] = {}
        for sd in self._table('sample_data'):
            if sd['is_key_frame']:
                cs = self.get('calibrated_sensor', sd['calibrated_sensor_token'])
                channel = self.get('sensor', cs['sensor_token'])['channel']
                self.get('sample', sd['sample_token'])['data'][channel] = sd['token']
        if verbose:
            print("Loaded %d samples of %d scenes from %s" % (len(self.sample), len(self.scene), self.table_root))

    def _table(self, name):
        if name not in self._tables:
            with open(os.path.join(self.table_root, name + '.json')) as f:
                self._tables[name] = json.load(f)
            self._index[name] = {rec['token']: i for i, rec in enumerate(self._tables[name])}
        return self._tables[name]

    @property
    def sample(self):
        return self._table('sample')

    @property
    def scene(self):
        return self._table('scene')

    def get(self, table_name, token):
        table = self._table(table_name)
        return table[self._index[table_name][token]]


def NuScenes(dataroot, version, *args, **kwargs):
    if (dataroot, version) not in GLOBAL_DICT:
        try:
            from nuscenes.nuscenes import NuScenes as NuSceneObj
        except ImportError:
            NuSceneObj = NuScenesTables
        GLOBAL_DICT[(dataroot, version)] = NuSceneObj(version=version, dataroot=dataroot, *args, **kwargs)
    return GLOBAL_DICT[(dataroot, version)]
