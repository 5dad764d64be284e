import json
import os


class NuScenes(object):
    TABLES = ['scene', 'sample', 'sample_data', 'ego_pose', 'calibrated_sensor', 'sensor']

    def __init__(self, version='v1.0-mini', dataroot='/data/sets/nuscenes', verbose=True, map_resolution=0.1):
        self.version, self.dataroot = version, dataroot
        for name in self.TABLES:
            with open(os.path.join(dataroot, version, name + '.json')) as f:
                setattr(self, name, json.load(f))
        self._token2ind = {name: {m['token']: i for i, m in enumerate(getattr(self, name))} for name in self.TABLES}
        for record in self.sample_data:
            cs_record = self.get('calibrated_sensor', record['calibrated_sensor_token'])
            sensor_record = self.get('sensor', cs_record['sensor_token'])
            record['sensor_modality'] = sensor_record['modality']
            record['channel'] = sensor_record['channel']
        for record in self.sample:
            record['data'] = {}
            record['anns'] = []
        for record in self.sample_data:
            if record['is_key_frame']:
                self.get('sample', record['sample_token'])['data'][record['channel']] = record['token']

    def get(self, table_name, token):
        return getattr(self, table_name)[self._token2ind[table_name][token]]
